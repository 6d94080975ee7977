"""ctypes binding of the joint importance-weighted extension of ``libprobnmn_hip.so`` (``pnmn_importance_bound_joint``,
csrc/importance_bound.hip), derived from include/probnmn_importance_joint.h as ``_hip_importance`` derives its own: ``lib()``
returns the handle ``_hip.lib()`` returns with the extension's entry point bound onto it as well."""
from probnmn._hip_extension import Extension

_extension = Extension("probnmn_importance_joint.h")
HEADER_PATH = _extension.header_path
SIGNATURES, RESTYPES = _extension.signatures, _extension.restypes
lib = _extension.lib
