"""Static compiler for prefix CLEVR programs.

The reference interprets each program token-by-token inside a ``try/except`` and calls any
exception "invalid program" (reference: probnmn/models/nmn.py:197-238).  On the GPU that would
also swallow genuine kernel failures, so here validity is decided *before* anything is
launched, by tracking only the channel count of the two registers the interpreter has
(``output`` and ``saved_output``); the rules are SURVEY.md App. C, which were checked
against the reference interpreter case by case (tests/golden/nmn_validity.json).

A compiled program is a short list of :class:`ModuleCall` s in execution order (the
reference walks the token sequence right-to-left) over *values*:

    value 0 = FEAT   the example's stem output, ``module_channels`` channels
    value 1 = ONES   the all-ones single-channel attention that ``scene`` produces
    value k>=2       output of call ``k-2``
"""
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

from probnmn import _hip

# token kinds
SKIP, SCENE, AND, OR, CMP, ATT, QUERY, REL, SAME = range(9)
KIND_NAMES = ["skip", "scene", "and", "or", "comparison", "attention", "query", "relate", "same"]

FEAT = 0
ONES = 1

_PLACEHOLDERS = {"@@PADDING@@", "@@UNKNOWN@@", "@start@", "@end@", "unique"}


def classify_token(token: str) -> int:
    """Token -> module kind, in the same test order as the reference's constructor
    (reference: probnmn/models/nmn.py:87-111) -- the order matters ("equal" before "query")."""
    if token in _PLACEHOLDERS:
        return SKIP
    if token == "scene":
        return SCENE
    if token == "intersect":
        return AND
    if token == "union":
        return OR
    if "equal" in token or token in ("less_than", "greater_than"):
        return CMP
    if "query" in token or token in ("exist", "count"):
        return QUERY
    if "relate" in token:
        return REL
    if "same" in token:
        return SAME
    return ATT


@dataclass(frozen=True)
class ModuleCall:
    kind: int  # AND .. SAME
    token: int  # program-vocabulary index (selects the weights)
    a: int  # first operand value id  (AND/OR/CMP: ``output``; others: the attention)
    b: int  # second operand value id (AND/OR/CMP: ``saved_output``; others: FEAT)
    a_channels: int
    b_channels: int
    out_channels: int


TOKEN_ROW = 48  # calls per program of the fixed-width token rows the scheduler stacks (longer programs: a copy loop)


class CompiledProgram:
    """valid / calls / result of one program.  ``calls`` (a tuple of :class:`ModuleCall`) is built on
    first use when the program came out of the batch compiler as an int32 table ``[n_calls, 7]``
    (kind, token, a, b, a_channels, b_channels, out_channels) -- the scheduler only needs the table."""

    __slots__ = ("valid", "result", "_raw", "_calls", "_template_id", "_template_owner", "_tokens", "_tokens_row", "_skey")

    def __init__(self, valid: bool, calls: Tuple[ModuleCall, ...] = (), result: int = FEAT, raw=None):
        self.valid = valid
        self.result = result  # value id of the final output (FEAT for an empty program)
        self._raw = raw
        self._calls = None if raw is not None else tuple(calls)  # empty when invalid
        self._template_id = None
        self._template_owner = None
        self._tokens = None
        self._tokens_row = None
        self._skey = None  # bytes of the call table with the token column zeroed (the scheduler's template key)

    @property
    def calls(self) -> Tuple[ModuleCall, ...]:
        if self._calls is None:
            self._calls = tuple(ModuleCall(*row) for row in self._raw.tolist())
        return self._calls

    def table(self):
        """int32 [n_calls, 7], the calls as rows."""
        if self._raw is None:
            import numpy as np

            self._raw = np.asarray([[c.kind, c.token, c.a, c.b, c.a_channels, c.b_channels, c.out_channels]
                                    for c in self._calls], dtype=np.int32).reshape(-1, 7)
        return self._raw

    def __eq__(self, other):
        return (isinstance(other, CompiledProgram) and self.valid == other.valid and self.result == other.result
                and self.calls == other.calls)

    def __repr__(self):
        return "CompiledProgram(valid=%r, calls=%r, result=%r)" % (self.valid, self.calls, self.result)


class ProgramCompiler:
    def __init__(self, index_to_token: Dict[int, str], module_channels: int = 128):
        self.module_channels = module_channels
        size = max(index_to_token) + 1
        self.kinds: List[int] = [SKIP] * size
        for idx, tok in index_to_token.items():
            self.kinds[idx] = classify_token(tok)
        self._cache: Dict[Tuple[int, ...], CompiledProgram] = {}
        self._bytes_cache: Dict[bytes, CompiledProgram] = {}
        self._kinds_array = None
        self._invalid = CompiledProgram(False, (), FEAT)
        self._automata: Dict[Tuple[int, ...], "DecodingAutomaton"] = {}

    def compile(self, tokens: Sequence[int]) -> CompiledProgram:
        key = tuple(int(t) for t in tokens)
        hit = self._cache.get(key)
        if hit is None:
            hit = self._compile(key)
            self._cache[key] = hit
        return hit

    def compile_batch(self, programs) -> List[CompiledProgram]:
        """``programs``: (B, T) integer array (numpy), already on the host.  Programs seen before
        come from a cache keyed by their bytes; the others are compiled together by the library's
        host routine (``pnmn_compile_programs``, the same rules as ``_compile``)."""
        import numpy as np

        from probnmn import _hip

        arr = np.ascontiguousarray(programs, dtype=np.int64)
        if arr.ndim != 2:
            raise ValueError("programs must be (batch, length), got shape %s" % (arr.shape,))
        cache = self._bytes_cache
        if len(cache) > 500000:  # bounded: sampled programs keep arriving for the whole training run
            cache.clear()
        keys = [row.tobytes() for row in arr]
        out = [cache.get(k) for k in keys]
        miss = [i for i, hit in enumerate(out) if hit is None]
        if miss:
            sub = np.ascontiguousarray(arr[miss])
            n, length = sub.shape
            if self._kinds_array is None:
                self._kinds_array = np.asarray(self.kinds, dtype=np.int32)
            valid = np.empty(n, np.uint8)
            n_calls = np.empty(n, np.int32)
            calls = np.empty((n, max(length, 1), 7), np.int32)
            result = np.empty(n, np.int32)
            _hip.check(_hip.lib().pnmn_compile_programs(
                sub.ctypes.data, n, length, self._kinds_array.ctypes.data, self._kinds_array.size, self.module_channels,
                valid.ctypes.data, n_calls.ctypes.data, calls.ctypes.data, result.ctypes.data), "compile_programs")
            valid_l, n_l, res_l = valid.tolist(), n_calls.tolist(), result.tolist()
            # what the scheduler wants of a new program, for the whole batch at once: the structure key (call table
            # without the tokens) and the tokens as a zero-padded int64 row -- per program these were a fancy-indexed
            # copy, an astype and a zeros() each, 4 us x ~35 new programs per step on the way to the first launch
            width = max(length, TOKEN_ROW)
            used = np.arange(max(length, 1))[None, :] < n_calls[:, None]
            struct = np.where(used[:, :, None], calls, 0)
            rows = np.zeros((n, width), np.int64)
            rows[:, : struct.shape[1]] = struct[:, :, 1]
            struct[:, :, 1] = 0
            for j, i in enumerate(miss):
                key = keys[i]
                hit = cache.get(key)  # (the same new program may occur several times in the batch)
                if hit is None:
                    if valid_l[j]:
                        nj = n_l[j]
                        hit = CompiledProgram(True, result=res_l[j], raw=calls[j, :nj].copy())
                        hit._skey = struct[j, :nj].tobytes()
                        hit._tokens = rows[j, :nj]
                        if nj <= TOKEN_ROW:
                            hit._tokens_row = rows[j, :TOKEN_ROW]
                    else:
                        hit = self._invalid
                    cache[key] = hit
                out[i] = hit
        return out

    # ---------------------------------------------------------------------------------
    def _compile(self, tokens: Tuple[int, ...]) -> CompiledProgram:
        D = self.module_channels
        invalid = CompiledProgram(False, (), FEAT)
        out, out_c = FEAT, D
        saved: Optional[int] = None
        saved_c = 0
        calls: List[ModuleCall] = []
        nkinds = len(self.kinds)
        for tok in reversed(tokens):
            if tok < 0 or tok >= nkinds:
                return invalid  # the reference's vocabulary lookup would raise KeyError
            kind = self.kinds[tok]
            step = register_step(kind, out_c, saved_c if saved is not None else None, D)
            if step is None:
                return invalid
            if step is _UNCHANGED:
                continue
            oc, _ = step
            if kind == SCENE:
                saved, saved_c = out, out_c
                out, out_c = ONES, 1
                continue
            if kind in (AND, OR, CMP):
                calls.append(ModuleCall(kind, tok, out, saved, out_c, saved_c, oc))
            else:  # ATT / QUERY / REL / SAME take (FEAT, attention)
                calls.append(ModuleCall(kind, tok, out, FEAT, 1, D, oc))
            out, out_c = len(calls) + 1, oc
        if out_c != D:
            return invalid
        return CompiledProgram(True, tuple(calls), out)

    # ---------------------------------------------------------------------------------
    def decoding_automaton(self, exclude: Sequence[int] = ()) -> "DecodingAutomaton":
        """The validity rule as a left-to-right automaton over token classes, for grammar-constrained beam search
        (the tables of ``pnmn_attn_lstm_beam``): a token string is accepted exactly when ``compile`` calls it valid.

        ``_compile`` reads a program right to left and its verdict depends on the channel counts of the two registers
        alone -- a small deterministic machine over ``register_step``.  A decoder emits left to right, so this is the
        reversed machine, determinised by subset construction: the subset after a prefix is the set of register states
        from which reading the prefix reversed ends with D output channels.  It starts as the set of accepting register
        states, is accepting when it holds the initial register state (D channels, nothing saved), and the empty subset
        is the dead state.  Token kinds with the same column share a class.  ``min_left`` counts only tokens a decoder
        may emit: every vocabulary index outside ``exclude`` (pad / unk / start / end)."""
        key = tuple(sorted(set(int(t) for t in exclude)))
        hit = self._automata.get(key)
        if hit is None:
            hit = self._automata[key] = _build_automaton(self.kinds, self.module_channels, key)
        return hit


_UNCHANGED = object()  # register_step: the token leaves both registers as they are


def register_step(kind: int, out_c: int, saved_c: Optional[int], D: int):
    """One token of the interpreter on the channel counts of its two registers (``saved_c`` None: nothing saved yet):
    ``None`` when the token is invalid here, ``_UNCHANGED`` for a skipped token, else the new (out_c, saved_c)."""
    if kind == SKIP:
        return _UNCHANGED
    if kind == SCENE:
        return 1, out_c
    if kind in (AND, OR):
        if saved_c is None:
            return None
        return max(out_c, saved_c), saved_c  # torch.min/max broadcast 1 <-> D channels
    if kind == CMP:
        if saved_c is None or out_c != D or saved_c != D:
            return None
        return D, saved_c
    # ATT / QUERY / REL / SAME take (FEAT, attention)
    if out_c != 1:
        return None
    return (D if kind == QUERY else 1), saved_c


MAX_AUTOMATON_STATES = _hip.BEAM_MAX_STATES   # PNMN_BEAM_MAX_STATES / PNMN_BEAM_MAX_CLASSES of include/probnmn_hip.h
MAX_AUTOMATON_CLASSES = _hip.BEAM_MAX_CLASSES
NO_COMPLETION = 255


class DecodingAutomaton:
    """``token_class`` [V], ``next_state`` [n_states, n_classes], ``min_left`` [n_states]: read-only contiguous uint8
    arrays, state 0 the start state (the layout ``pnmn_attn_lstm_beam`` takes)."""

    __slots__ = ("token_class", "next_state", "min_left")

    def __init__(self, token_class, next_state, min_left):
        import numpy as np

        arrays = []
        for a in (token_class, next_state, min_left):
            a = np.array(a, dtype=np.uint8, order="C")
            a.setflags(write=False)
            arrays.append(a)
        tc, ns, ml = arrays
        if tc.ndim != 1 or ns.ndim != 2 or ml.ndim != 1 or ns.shape[0] != ml.shape[0]:
            raise ValueError("token_class [V], next_state [n_states, n_classes], min_left [n_states]")
        if not (1 <= ns.shape[0] <= MAX_AUTOMATON_STATES and 1 <= ns.shape[1] <= MAX_AUTOMATON_CLASSES):
            raise ValueError("decoding automaton of %d states x %d classes: the beam kernel takes at most %d x %d"
                             % (ns.shape[0], ns.shape[1], MAX_AUTOMATON_STATES, MAX_AUTOMATON_CLASSES))
        if (tc.size and int(tc.max()) >= ns.shape[1]) or int(ns.max()) >= ns.shape[0]:
            raise ValueError("decoding automaton: a table entry is out of range")
        object.__setattr__(self, "token_class", tc)
        object.__setattr__(self, "next_state", ns)
        object.__setattr__(self, "min_left", ml)

    def __setattr__(self, name, value):
        raise AttributeError("DecodingAutomaton is immutable")

    @property
    def n_states(self) -> int:
        return self.next_state.shape[0]

    @property
    def n_classes(self) -> int:
        return self.next_state.shape[1]

    def accepts(self, tokens: Sequence[int]) -> bool:
        s = 0
        for t in tokens:
            if t < 0 or t >= self.token_class.size:
                return False
            s = int(self.next_state[s, self.token_class[t]])
        return int(self.min_left[s]) == 0


def _build_automaton(kinds: Sequence[int], D: int, exclude: Tuple[int, ...]) -> DecodingAutomaton:
    n_kinds = len(KIND_NAMES)
    # the register states _compile can be in: (out_c, saved_c), saved_c None before the first `scene`
    regs = [(o, s) for o in (1, D) for s in (None, 1, D)] if D != 1 else [(1, None), (1, 1)]
    initial = (D, None)

    def after(kind, reg):
        step = register_step(kind, reg[0], reg[1], D)
        return reg if step is _UNCHANGED else step

    # reading a prefix reversed = its LAST token first: extending the prefix by token x puts x in front of the reversed
    # string, so the new subset is {r : step(x, r) is in the old subset}
    start = frozenset(r for r in regs if r[0] == D)
    subsets, table = [start], []
    index = {start: 0}
    i = 0
    while i < len(subsets):
        row = []
        for kind in range(n_kinds):
            nxt = frozenset(r for r in regs if after(kind, r) in subsets[i])
            if nxt not in index:
                index[nxt] = len(subsets)
                subsets.append(nxt)
            row.append(index[nxt])
        table.append(row)
        i += 1
    n_states = len(subsets)
    # kinds with identical columns share a class
    columns = [tuple(table[s][k] for s in range(n_states)) for k in range(n_kinds)]
    class_of_column: Dict[Tuple[int, ...], int] = {}
    kind_class = [class_of_column.setdefault(col, len(class_of_column)) for col in columns]
    n_classes = len(class_of_column)
    if n_states > MAX_AUTOMATON_STATES or n_classes > MAX_AUTOMATON_CLASSES:
        raise ValueError("decoding automaton of %d states x %d classes: the beam kernel takes at most %d x %d"
                         % (n_states, n_classes, MAX_AUTOMATON_STATES, MAX_AUTOMATON_CLASSES))
    next_state = [[0] * n_classes for _ in range(n_states)]
    for k in range(n_kinds):
        for s in range(n_states):
            next_state[s][kind_class[k]] = table[s][k]
    token_class = [kind_class[k] for k in kinds]
    # fewest further tokens to an accepting subset, over the classes of tokens a decoder may emit
    emitted = sorted({token_class[t] for t in range(len(kinds)) if t not in exclude})
    min_left = [0 if initial in subsets[s] else NO_COMPLETION for s in range(n_states)]
    for _ in range(n_states):
        for s in range(n_states):
            for c in emitted:
                via = min_left[next_state[s][c]]
                if via != NO_COMPLETION and via + 1 < min_left[s]:
                    min_left[s] = via + 1
    return DecodingAutomaton(token_class, next_state, min_left)
