"""ctypes binding of the grammar extension of ``libprobnmn_hip.so``, derived from include/probnmn_grammar.h.

The core ABI (include/probnmn_hip.h: its version, entry points, records and launch ops) is pinned; the entry points of
``csrc/grammar_logits.hip`` are declared in a header of their own, written to the same declaration conventions, which
``_hip.read_header`` reads as it is.  ``lib()`` returns the handle ``_hip.lib()`` returns with these entry points bound onto
it as well; ``_hip.SIGNATURES`` / ``RECORDS`` / ``CONSTANTS`` stay the core header's.  As everywhere in the package a
missing symbol is an error: there is no fallback."""
import os
from typing import Optional

from probnmn import _hip

HEADER_PATH = os.path.join(os.path.dirname(_hip.HEADER_PATH), "probnmn_grammar.h")

# name -> argtypes / restype of the extension's entry points (the header declares no record and no constant)
SIGNATURES, RESTYPES, _records, _constants = _hip.read_header(HEADER_PATH)
if _records or _constants:
    raise _hip.HipLibraryError("probnmn_grammar.h declares entry points only; records and constants belong to probnmn_hip.h")

_bound: Optional[object] = None


def lib():
    """``_hip.lib()`` with the extension's entry points bound (``AttributeError`` if the library does not export one)."""
    global _bound
    handle = _hip.lib()
    if _bound is not handle:
        for name, argtypes in SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = RESTYPES[name]
            fn.argtypes = list(argtypes)
        _bound = handle
    return handle
