"""ctypes binding of ``libprobnmn_hip.so``, derived from its C header (include/probnmn_hip.h).

The header is the one statement of the ABI.  ``read_header`` parses it when this module is imported and everything the
package binds comes out of that: ``SIGNATURES`` / ``RESTYPES`` (every ``pnmn_*`` prototype), one numpy record dtype per
``typedef struct ... pnmn_x;`` (``pnmn_conv_item`` -> ``CONV_ITEM``), one per host argument block ``struct pnmn_x { ... };``
(``HOST_BLOCKS``; ``pnmn_sampling_filter`` -> ``SAMPLING_FILTER``) and one integer per ``#define PNMN_NAME``
(``PNMN_OP_CONV`` -> ``OP_CONV``).  A new entry point, record or constant is therefore added in the header and in its
``.hip`` file, nowhere else; tests/test_abi.py holds the result against the C++ compiler's own view of the header.

The library is the product: if it is missing, or a call fails, this module raises -- there is no
CPU or eager-PyTorch fallback anywhere in the package.  ``torch`` is imported first on purpose:
the library links ``libamdhip64.so.7`` and must bind to the HIP runtime torch already loaded, so
that torch's stream handles and device pointers are valid inside it.
"""
import ctypes
import os
import re
import time
from typing import Dict, Optional

import numpy as np
import torch  # noqa: F401  (must precede the dlopen below)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PNMN_LIB") or os.path.join(os.path.dirname(_HERE), "lib", "libprobnmn_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "probnmn_hip.h")


class HipLibraryError(RuntimeError):
    pass


_lib: Optional[ctypes.CDLL] = None

# C scalar type -> (ctypes type as a parameter or return value, numpy type as a record field).  Closed on purpose: a type
# that is not listed here fails the import, it is never guessed.  Anything declared with a `*` is a pointer.
_C_SCALARS = {
    "int": (ctypes.c_int, np.int32),
    "int32_t": (ctypes.c_int32, np.int32),
    "uint32_t": (ctypes.c_uint32, np.uint32),
    "int64_t": (ctypes.c_int64, np.int64),
    "uint64_t": (ctypes.c_uint64, np.uint64),
    "float": (ctypes.c_float, np.float32),
    "double": (ctypes.c_double, np.float64),
}


HOST_BLOCKS: Dict[str, np.dtype] = {}  # `struct pnmn_x { ... };` of the header last read -> aligned numpy dtype


def read_header(path: str = HEADER_PATH, text: Optional[str] = None):
    """(signatures, restypes, records, constants) of the C header at ``path`` (or of ``text``), following the declaration
    conventions stated at its top: prototype name -> argtypes tuple and -> return type, struct name -> aligned numpy
    dtype (pointer fields as uint64), ``PNMN_*`` -> int.  A ``pnmn_`` declaration it cannot read raises, naming it.
    Host argument blocks (``struct pnmn_x { ... };`` without a typedef) are not records: their dtypes go to ``HOST_BLOCKS``."""
    if text is None:
        try:
            with open(path) as f:
                text = f.read()
        except OSError as e:
            raise HipLibraryError("cannot read %s (%s): the binding is derived from this header" % (path, e))
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)

    def scalar(ctype: str, decl: str, which: int):
        if ctype not in _C_SCALARS:
            raise HipLibraryError("probnmn_hip.h: type `%s` in `%s` is not one the binding knows (%s)"
                                  % (ctype, " ".join(decl.split()), ", ".join(_C_SCALARS)))
        return _C_SCALARS[ctype][which]

    constants: Dict[str, int] = {}
    for line in re.findall(r"^[ \t]*#[ \t]*define[ \t]+PNMN_.*$", text, flags=re.M):
        m = re.fullmatch(r"\s*#\s*define\s+(PNMN_\w+)\s+(?:(\d+)|\((-\d+)\))\s*", line)
        if m is None:
            raise HipLibraryError("probnmn_hip.h: `%s` is not an integer constant" % line.strip())
        constants[m[1]] = int(m[2] or m[3])

    def record(body: str, name: str) -> np.dtype:
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            # `const float *a, *b` or `int32_t n, p[8]`: a type, then declarators; a `*` makes its declarator a pointer
            words = re.sub(r"\bconst\b", " ", decl).replace("*", " * ").split(None, 1)
            declarators = [re.fullmatch(r"\s*(\*?)\s*(\w+)\s*(?:\[\s*(\w+)\s*\])?\s*", d) for d in words[-1].split(",")]
            if len(words) != 2 or None in declarators:
                raise HipLibraryError("probnmn_hip.h: cannot read the field `%s` of %s" % (decl, name))
            for star, field, length in (d.groups() for d in declarators):
                kind = np.uint64 if star else scalar(words[0], "%s; /* %s */" % (decl, name), 1)
                if length is None:
                    fields.append((field, kind))
                elif length.isdigit() or length in constants:
                    fields.append((field, kind, (int(length) if length.isdigit() else constants[length],)))
                else:
                    raise HipLibraryError("probnmn_hip.h: array length `%s` of `%s` in %s is neither a number nor a "
                                          "#define above it" % (length, decl, name))
        return np.dtype(fields, align=True)

    records: Dict[str, np.dtype] = {}
    for m in re.finditer(r"\btypedef\b(?:\s+struct\s*\w*\s*\{([^{}]*)\}\s*(pnmn_\w+)\s*;)?", text):
        if m[2] is None:
            raise HipLibraryError("probnmn_hip.h: cannot read the record at `%s`: a record is `typedef struct [tag] { ... } "
                                  "pnmn_x;`" % " ".join(text[m.start():m.start() + 60].split()))
        records[m[2]] = record(m[1], m[2])
    # host argument blocks, `struct pnmn_x { ... };` without a typedef: the same field kinds, kept beside the records
    HOST_BLOCKS.update({m[1]: record(m[2], m[1]) for m in re.finditer(r"^[ \t]*struct\s+(pnmn_\w+)\s*\{([^{}]*)\}\s*;", text, flags=re.M)})

    signatures: Dict[str, tuple] = {}
    restypes = {}
    for m in re.finditer(r"^(int|int64_t)\s+(pnmn_\w+)\s*\(([^()]*)\)\s*;", text, flags=re.M):
        params = [p.strip() for p in m[3].split(",")]
        argtypes = []
        for p in [] if params in (["void"], [""]) else params:
            words = re.sub(r"\b(const|struct)\b", " ", p).split()
            if "*" in p:
                argtypes.append(ctypes.c_void_p)
            elif len(words) == 2:
                argtypes.append(scalar(words[0], "%s /* %s */" % (p, m[2]), 0))
            else:
                raise HipLibraryError("probnmn_hip.h: cannot read the parameter `%s` of %s" % (p, m[2]))
        signatures[m[2]] = tuple(argtypes)
        restypes[m[2]] = _C_SCALARS[m[1]][0]
    for m in re.finditer(r"\b(pnmn_\w+)\s*\(", text):
        if m[1] not in signatures:
            raise HipLibraryError("probnmn_hip.h: cannot read the declaration of %s: a prototype is `int` or `int64_t` at "
                                  "the start of a line, the name, the parameters, `);`" % m[1])
    return signatures, restypes, records, constants


# name -> argtypes / restype of every entry point, C struct name -> record dtype, PNMN_* -> value
SIGNATURES, RESTYPES, RECORDS, CONSTANTS = read_header()
globals().update({name[len("pnmn_"):].upper(): dtype for name, dtype in RECORDS.items()})  # pnmn_conv_item -> CONV_ITEM
globals().update({name[len("pnmn_"):].upper(): dtype for name, dtype in HOST_BLOCKS.items()})  # struct pnmn_sampling_filter -> SAMPLING_FILTER
globals().update({name[len("PNMN_"):]: value for name, value in CONSTANTS.items()})        # PNMN_OP_CONV -> OP_CONV, ...
GEMM_A_T, GEMM_B_T, GEMM_ACC = (CONSTANTS["PNMN_GEMM_" + n] for n in ("A_TRANSPOSED", "B_TRANSPOSED", "ACCUMULATE"))
ABI_VERSION = CONSTANTS["PNMN_ABI_VERSION"]  # what pnmn_abi_version() of a library built from this header returns
ITEM_SIZES = {name: (dtype, dtype.itemsize) for name, dtype in RECORDS.items()}


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HipLibraryError(
                "libprobnmn_hip.so not found at %s -- build it with `python -c 'import "
                "__graft_entry__ as g; g.build()'` (hipcc --offload-arch=gfx950); there is no "
                "fallback path" % LIB_PATH
            )
        handle = ctypes.CDLL(LIB_PATH)
        for name, argtypes in SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError if the symbol is not exported
            fn.restype = RESTYPES[name]
            fn.argtypes = list(argtypes)
        if handle.pnmn_abi_version() != ABI_VERSION:  # (same symbol names, other argument lists: never call into it)
            raise HipLibraryError("%s has ABI version %d, this package binds version %d -- rebuild the library"
                                  % (LIB_PATH, handle.pnmn_abi_version(), ABI_VERSION))
        _lib = handle
    return _lib


_TRACE = None  # debugging aid (PNMN_TRACE_LAUNCHES=<seconds>): see _start_trace


def check(code: int, what: str) -> None:
    if code != 0:
        kind = "argument/shape error" if code < 0 else "hipError_t"
        raise HipLibraryError("%s failed: %s %d" % (what, kind, code))
    if _TRACE is not None:
        stream = torch.cuda.current_stream()
        ev = torch.cuda.Event()
        ev.record(stream)
        _TRACE.append((what, stream.cuda_stream, ev))
        del _TRACE[:-4000]


def mark(what: str) -> None:
    """A named point on the current stream's timeline (only when launch tracing is on)."""
    if _TRACE is not None:
        check(0, "mark: " + what)


def _start_trace(seconds: float) -> None:
    """Every library launch leaves an event behind; a watchdog thread reports, `seconds` after start, the
    first launch of each stream whose event has not completed -- i.e. the kernel a stalled GPU is stuck in
    (or waiting behind).  For diagnosing cross-stream stalls; costs one event per launch."""
    import sys
    import threading

    global _TRACE
    _TRACE = []

    def watch():
        time.sleep(seconds)
        per_stream = {}
        for what, stream, ev in list(_TRACE):
            st = per_stream.setdefault(stream, {"done": None, "stuck": None, "pending": 0})
            if ev.query():
                if st["stuck"] is None:
                    st["done"] = what
            else:
                st["pending"] += 1
                if st["stuck"] is None:
                    st["stuck"] = what
        for stream, st in per_stream.items():
            print("[pnmn trace] stream %#x: last completed launch = %s; first incomplete = %s (%d launches pending)"
                  % (stream, st["done"], st["stuck"], st["pending"]), file=sys.stderr, flush=True)

    threading.Thread(target=watch, daemon=True).start()


if os.environ.get("PNMN_TRACE_LAUNCHES"):
    _start_trace(float(os.environ["PNMN_TRACE_LAUNCHES"]))


class LaunchList:
    """A sequence of grouped launches for ``pnmn_run_launches`` (one binding call instead of one per launch).
    Rows are kept as tuples of eight 64-bit words -- the byte image of ``pnmn_launch`` (a, b, c, op | n << 32,
    p0 | p1 << 32, ...) -- and turned into one array when the list runs."""

    def __init__(self):
        self._rows = []

    def add(self, op: int, n: int, a: int, b: int = 0, c: int = 0, p=()) -> None:
        q = tuple(p) + (0,) * (8 - len(p))
        self._rows.append((a, b, c, op | (n << 32), q[0] | (q[1] << 32), q[2] | (q[3] << 32), q[4] | (q[5] << 32),
                           q[6] | (q[7] << 32)))

    def __len__(self) -> int:
        return len(self._rows)

    def run(self, stream: int, what: str) -> None:
        if self._rows:
            rec = np.array(self._rows, dtype=np.uint64)
            check(lib().pnmn_run_launches(rec.ctypes.data, len(self._rows), stream), what)
            self._rows = []


def decoder_workspace_bytes(rows, backward: bool) -> int:
    """``pnmn_attn_lstm_group_workspace_bytes`` for decoder passes of ``rows[i]`` rows each in one call (1-3 of them)."""
    r = np.asarray(rows, np.int32)
    return int(lib().pnmn_attn_lstm_group_workspace_bytes(r.ctypes.data, len(r), 1 if backward else 0))


def stream_ptr(device: torch.device) -> int:
    """Raw handle of torch's current stream on ``device`` (every kernel call needs it: the raw query costs a
    fraction of building a ``torch.cuda.Stream`` object, ~6 us x 80 calls per step)."""
    idx = device.index
    if idx is None:
        idx = torch.cuda.current_device()
    return torch._C._cuda_getCurrentRawStream(idx)


class _PinnedRing:
    """Reusable page-locked staging buffers for small host->device copies.

    ``Tensor.pin_memory()`` costs a hipHostMalloc (milliseconds) per call; a training step uploads
    its work lists every iteration, so staging memory is allocated once and recycled.  A slot is
    reused only after the copy that last read it has completed (event), which lets the host run
    several steps ahead of the GPU without overwriting bytes that are still to be copied.
    Two size classes: many fixed 16 KiB slots carved out of one allocation for the short records (optimiser
    items, derived-parameter jobs, index vectors: a copy is stream ordered, so waiting for a slot means
    waiting for everything queued before its last use -- with few slots the host could never run ahead), and a
    few growable slots for the per-step work lists."""

    SMALL, SMALL_SLOTS = 16 << 10, 64

    def __init__(self, slots: int = 6):
        self._bufs = [None] * slots
        self._events = [None] * slots
        self._next = 0
        self._small = None
        self._big = 16 << 20
        self._small_events = [None] * self.SMALL_SLOTS
        self._small_next = 0
        self.wait_seconds = 0.0  # time the host spent blocked on the GPU (diagnostic)

    def _wait(self, ev) -> None:
        if ev is not None and not ev.query():
            t0 = time.perf_counter()
            ev.synchronize()  # the host is far ahead of the GPU: wait for the slot
            self.wait_seconds += time.perf_counter() - t0

    def stage(self, raw, device: torch.device, total: int = -1) -> torch.Tensor:
        """``raw``: a uint8 array, or (with ``total`` = their summed size) a list of (offset, uint8 array) pieces that
        are copied straight into the pinned slot (no concatenated host copy first)."""
        pieces = None
        if total >= 0:
            pieces, n = raw, total
        else:
            n = raw.size
        if n <= self.SMALL:
            if self._small is None:
                self._small = torch.empty(self.SMALL * self.SMALL_SLOTS, dtype=torch.uint8).pin_memory()
            i = self._small_next
            self._small_next = (i + 1) % self.SMALL_SLOTS
            events, buf = self._small_events, self._small[i * self.SMALL:(i + 1) * self.SMALL]
        else:
            i = self._next
            self._next = (i + 1) % len(self._bufs)
            events, buf = self._events, self._bufs[i]
        self._wait(events[i])
        if buf is None or buf.numel() < n:
            # a hipHostMalloc costs milliseconds (19 ms seen for 0.5 MB): the growable slots share one size, 16 MB to
            # begin with -- several times the longest work list of any configuration measured (3 MB: 28x28 maps,
            # 40-token programs) -- that doubles when a list outgrows it; a slot is replaced when it is next used.
            # (Sized to the list at hand, every slot regrew whenever a step's sampled programs made a longer list than
            # that slot had seen: a 4 ms tail on one step in five at 128 questions.)
            while self._big < n:
                self._big *= 2
            buf = torch.empty(self._big, dtype=torch.uint8).pin_memory()
            self._bufs[i] = buf
        if pieces is None:
            buf.numpy()[:n] = raw
        else:
            view = buf.numpy()
            for off, piece in pieces:
                view[off:off + piece.size] = piece
        out = buf[:n].to(device, non_blocking=True)
        if events[i] is None:
            events[i] = torch.cuda.Event()
        events[i].record(torch.cuda.current_stream(device))
        return out


_rings: Dict[int, _PinnedRing] = {}


def _ring(device: torch.device) -> _PinnedRing:
    idx = device.index if device.index is not None else torch.cuda.current_device()
    r = _rings.get(idx)
    if r is None:
        r = _rings[idx] = _PinnedRing()
    return r


def ring_wait_seconds() -> float:
    """Total time the host has been blocked waiting for staging slots (i.e. for the GPU)."""
    return sum(r.wait_seconds for r in _rings.values())


def to_device(records: np.ndarray, device: torch.device) -> torch.Tensor:
    """Copy a numpy (record) array into device memory asynchronously through the pinned ring.
    Returns a uint8 tensor owning the device copy; stream order protects it until the kernels that
    read it have run."""
    if device.type != "cuda":
        raise HipLibraryError("probnmn HIP kernels need a cuda (ROCm) device, got %s" % device)
    raw = np.ascontiguousarray(records).view(np.uint8).reshape(-1)
    return _ring(device).stage(raw, device)


def pieces_to_device(pieces, total: int, device: torch.device) -> torch.Tensor:
    """``to_device`` of the concatenation of (offset, uint8 array) pieces laid out in ``total`` bytes (gaps between
    pieces carry whatever the staging slot held)."""
    if device.type != "cuda":
        raise HipLibraryError("probnmn HIP kernels need a cuda (ROCm) device, got %s" % device)
    return _ring(device).stage(pieces, device, total)


def small_to_device(values, dtype: torch.dtype, device: torch.device) -> torch.Tensor:
    """A short Python list -> device tensor WITHOUT synchronising the stream (``torch.tensor(...,
    device=cuda)`` copies from pageable memory and waits for all queued work first)."""
    host = torch.tensor(values, dtype=dtype)
    if host.numel() == 0:
        return torch.empty(0, dtype=dtype, device=device)
    raw = host.view(torch.uint8).numpy() if dtype != torch.bool else host.numpy().view(np.uint8)
    return to_device(raw, device).view(dtype)
