"""ctypes binding of the importance-weighted extension of ``libprobnmn_hip.so`` (``pnmn_importance_bound``,
csrc/importance_bound.hip), derived from include/probnmn_importance.h as ``_hip_grammar`` derives its own: ``lib()`` returns
the handle ``_hip.lib()`` returns with the extension's entry point bound onto it as well."""
from probnmn._hip_extension import Extension

_extension = Extension("probnmn_importance.h")
HEADER_PATH = _extension.header_path
SIGNATURES, RESTYPES = _extension.signatures, _extension.restypes
lib = _extension.lib
