"""``pnmn_trunk_last_attention`` (csrc/host_trunk.hip): where in the activation arena the one-channel map of every program
token's module call lies -- against offsets worked out here from the planner's specification (``schedule.build_template``
and the cumulative template sizes), and against the rules for "no map" one by one.  No GPU: ``launch = 0`` plans on the host."""
import numpy as np

from probnmn import _hip
from probnmn.runtime import program_compiler as pc
from probnmn.runtime import schedule

from fixtures import encode_programs
from test_schedule import C, HW, _scheduler
from test_trunk_planner import _planner, _run

LENGTH = 26
CASES = {
    "chain": "query_color unique filter_shape[cube] relate[left] unique filter_color[red] scene",
    "intersect": "count intersect filter_color[red] relate[left] unique filter_shape[cube] scene filter_size[large] "
                 "relate[right] unique filter_material[rubber] scene",
    "union": "count union filter_color[red] scene filter_shape[cube] scene",
    "same": "query_shape unique same_color unique filter_size[small] filter_material[metal] scene",
    "comparison": "equal_color query_color unique filter_shape[cube] scene query_color unique filter_size[large] "
                  "relate[front] unique filter_material[metal] scene",
    "wide_and": "intersect count scene count scene",
    "dead": "count filter_color[red] scene count filter_shape[cube] scene count scene",
    "invalid": "filter_color[red] query_color scene",
    "padded": "@start@ count filter_color[red] scene @end@",
    "empty": "",
}
NAMES = list(CASES)


def _expected(comp, programs):
    """[B, T] offsets from the specification: call k is the k-th module token from the right; its map is the output slot of
    its last primitive when that is a small arena slot; arena blocks of the valid programs follow one another."""
    want = -np.ones(programs.shape, np.int64)
    base = 0
    for i, (row, prog) in enumerate(zip(programs, comp.compile_batch(programs))):
        if not prog.valid:
            continue
        positions = [p for p in range(len(row) - 1, -1, -1) if comp.kinds[row[p]] not in (pc.SKIP, pc.SCENE)]
        assert len(positions) == len(prog.calls)
        t = schedule.build_template(prog, HW, C)
        for k, call in enumerate(prog.calls):
            prims = t.table[t.table[:, schedule.C_CALL] == k]
            if len(prims) and prims[-1, schedule.C_OK] == schedule.L_SLOT and call.out_channels != C:
                want[i, positions[k]] = base + prims[-1, schedule.C_OO]
        base += t.size
    return want, base


def _ask(planner, B, length, capacity=None):
    out = np.full(B * length + 3, -7, np.int64)
    n = _hip.lib().pnmn_trunk_last_attention(planner, out.ctypes.data, B * length if capacity is None else capacity)
    return n, out


def test_offsets_equal_the_specifications_and_the_no_map_rules_hold():
    v, comp, s = _scheduler()
    stoi = v.get_token_to_index_vocabulary("programs")
    planner = _planner(s, comp)
    assert _ask(planner, 0, 0)[0] == 0  # nothing planned yet: nothing to ask about
    programs = encode_programs(CASES.values(), stoi, length=LENGTH).numpy()
    rc, io, *_ = _run(planner, programs)
    assert rc == 0
    B = len(programs)
    n, raw = _ask(planner, B, LENGTH)
    assert n == B * LENGTH and raw[n:].tolist() == [-7, -7, -7]  # nothing written past n entries
    got = raw[:n].reshape(B, LENGTH)
    want, arena = _expected(comp, programs)
    assert arena == io["arena_floats"]
    assert np.array_equal(got, want)

    def tokens_with_maps(name):
        row = got[NAMES.index(name)]
        return [(p, CASES[name].split()[p]) for p in range(LENGTH) if row[p] >= 0]

    # the rules one by one.  Skipped tokens (unique, @start@, @end@, padding), `scene`, and wide outputs (query, count) have none
    assert tokens_with_maps("chain") == [(2, "filter_shape[cube]"), (3, "relate[left]"), (5, "filter_color[red]")]
    assert tokens_with_maps("intersect") == [(1, "intersect"), (2, "filter_color[red]"), (3, "relate[left]"), (5, "filter_shape[cube]"),
                                             (7, "filter_size[large]"), (8, "relate[right]"), (10, "filter_material[rubber]")]
    assert tokens_with_maps("union") == [(1, "union"), (2, "filter_color[red]"), (4, "filter_shape[cube]")]
    assert tokens_with_maps("same") == [(2, "same_color"), (4, "filter_size[small]"), (5, "filter_material[metal]")]
    # a comparison of two queries: only the filters and the relate below them
    assert tokens_with_maps("comparison") == [(3, "filter_shape[cube]"), (7, "filter_size[large]"), (8, "relate[front]"),
                                              (10, "filter_material[metal]")]
    assert tokens_with_maps("wide_and") == []  # and / or with a wide operand is wide
    # executed right to left, each `scene` saves the count before it and only the LAST chain reaches the result:
    # filter_shape[cube] (position 4) is valid, one-channel and never executed
    assert tokens_with_maps("dead") == [(1, "filter_color[red]")]
    assert not comp.compile(programs[NAMES.index("invalid")]).valid and tokens_with_maps("invalid") == []
    assert tokens_with_maps("padded") == [(2, "filter_color[red]")]
    assert tokens_with_maps("empty") == []

    live = got[got >= 0]
    assert live.size == 22 and len(set(live.tolist())) == live.size  # every map has a slot of its own
    assert np.all(live % 64 == 0) and np.all(live + HW <= io["arena_floats"])

    # arguments: a null planner, a short capacity, a null array
    assert _hip.lib().pnmn_trunk_last_attention(None, raw.ctypes.data, raw.size) == _hip.EINVAL
    assert _ask(planner, B, LENGTH, capacity=B * LENGTH - 1)[0] == _hip.EINVAL
    assert _hip.lib().pnmn_trunk_last_attention(planner, None, B * LENGTH) == _hip.EINVAL

    # a second batch (programs now come from the planner's cache, in another order, at another length) replaces the first
    again = np.concatenate([programs[::-1], np.zeros((B, 2), np.int64)], axis=1)
    assert _run(planner, again)[0] == 0
    n, raw = _ask(planner, B, LENGTH + 2)
    assert n == B * (LENGTH + 2)
    assert np.array_equal(raw[:n].reshape(B, LENGTH + 2), _expected(comp, again)[0])
    # a call that fails leaves nothing to ask about
    assert _run(planner, programs, capacity=10)[0] == _hip.EAGAIN
    assert _ask(planner, B, LENGTH)[0] == 0
    _hip.lib().pnmn_trunk_planner_destroy(planner)
