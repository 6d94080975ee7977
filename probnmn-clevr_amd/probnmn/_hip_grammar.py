"""ctypes binding of the grammar extension of ``libprobnmn_hip.so``, derived from include/probnmn_grammar.h.

The core ABI (include/probnmn_hip.h: its version, entry points, records and launch ops) is pinned; the entry points of
``csrc/grammar_logits.hip`` are declared in a header of their own, written to the same declaration conventions, which
``_hip.read_header`` reads as it is.  ``lib()`` returns the handle ``_hip.lib()`` returns with these entry points bound onto
it as well; ``_hip.SIGNATURES`` / ``RECORDS`` / ``CONSTANTS`` stay the core header's.  As everywhere in the package a
missing symbol is an error: there is no fallback.  (The reading and the binding: ``_hip_extension.Extension``.)"""
from probnmn._hip_extension import Extension

_extension = Extension("probnmn_grammar.h")
HEADER_PATH = _extension.header_path
SIGNATURES, RESTYPES = _extension.signatures, _extension.restypes  # name -> argtypes / restype of the extension's entry points
lib = _extension.lib
