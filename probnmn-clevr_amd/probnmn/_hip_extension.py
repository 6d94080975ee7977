"""What the extension headers of ``libprobnmn_hip.so`` share (include/probnmn_grammar.h, include/probnmn_importance.h): the
core ABI (include/probnmn_hip.h) is pinned, so entry points added to the library are declared in headers of their own,
written to the core header's declaration conventions, which ``_hip.read_header`` reads as they are.  An ``Extension`` reads
one such header and binds its entry points onto the handle ``_hip.lib()`` returns; ``_hip.SIGNATURES`` / ``RECORDS`` /
``CONSTANTS`` stay the core header's.  As everywhere in the package a missing symbol is an error: there is no fallback."""
import os
from typing import Optional

from probnmn import _hip


class Extension:
    def __init__(self, header_name: str):
        self.header_path = os.path.join(os.path.dirname(_hip.HEADER_PATH), header_name)
        # name -> argtypes / restype of the extension's entry points (an extension declares no record and no constant)
        self.signatures, self.restypes, records, constants = _hip.read_header(self.header_path)
        if records or constants:
            raise _hip.HipLibraryError("%s declares entry points only; records and constants belong to probnmn_hip.h" % header_name)
        self._bound: Optional[object] = None

    def lib(self):
        """``_hip.lib()`` with the extension's entry points bound (``AttributeError`` if the library does not export one)."""
        handle = _hip.lib()
        if self._bound is not handle:
            for name, argtypes in self.signatures.items():
                fn = getattr(handle, name)
                fn.restype = self.restypes[name]
                fn.argtypes = list(argtypes)
            self._bound = handle
        return handle
