"""GPU: states rendered into a caller-owned store at rows chosen by a device-side `dest`
(include/simaps_store.h, StateBatch.render_into, VectorEnvObservations.get_state_into), and the
mixed-configuration launch in bf16 / fp16 (MixedStateBatch.render(dtype=...)).

The oracle of every stack is the existing contiguous float32 render(), cast by torch on the CPU for the
16-bit types; every comparison is on integer views and exact.  The scenes are the golden one-env
scenes of tests/goldens.py (the mixed test: two one-env scenes of tests/test_gpu_mixed.py's
configurations), at most 4 agents per configuration.
"""
import os

import numpy as np
import pytest
import torch

import goldens as G

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ['f32', 'bf16', 'f16']
LAYOUTS = ['chw', 'hwc']
CFG = 'lifting_4-small_divider'
SPATIAL = 'lifting_4-small_divider-spatial'                 # C = 7: an odd pixel length in HWC
ALL = 'lifting_2_pushing_2-large_empty-all'                 # C = 10


@pytest.fixture(scope='module')
def S():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a GPU (run with -m gpu on an MI355X)')
    from simaps import _lib, batch, context, vector_env
    _lib.lib.simaps_fault_status(1)
    yield _lib, batch, context, vector_env
    _lib.lib.simaps_fault_status(1)


_GOLD = {}


def golden(cfg):
    """(scene, agents) of env 0 of tests/golden/scene_<cfg>.npz with every robot an agent: the goldens
    carry the maps of some agents only, the others get a copy of the first golden agent's (each robot
    maps the same room).  A fresh shallow copy of the scene."""
    if not _GOLD:
        for _, e, a, scene, _, z in G.scene_cases():
            if e == 0:
                stem = os.path.splitext(os.path.basename(z.zip.filename))[0][len('scene_'):]
                _GOLD.setdefault(stem, (scene, []))[1].append(a)
    scene, have = _GOLD[cfg]
    occ, ovh = scene['occupancy'].copy(), scene['overhead'].copy()
    for a in range(len(scene['robots'])):
        if a not in have:
            occ[a], ovh[a] = occ[have[0]], ovh[have[0]]
    return dict(scene, occupancy=occ, overhead=ovh), [(0, a) for a in range(len(scene['robots']))]


def _moved(scene):
    """The scene one step later: every robot turned and shifted a little (same maps)."""
    robots = [dict(r, heading=r['heading'] + 0.4, position=(r['position'][0] + 0.03, r['position'][1] - 0.02) +
                   tuple(r['position'][2:])) for r in scene['robots']]
    return dict(scene, robots=robots)


def ints(t):
    """The integer view of a float32 / bf16 / fp16 tensor, on the host."""
    t = t.detach().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu().numpy()


def cast(f32, dtype):
    """The oracle: torch's CPU cast of the float32 render, as integers."""
    return ints(f32.detach().cpu().to(dtype))


def sentinel_store(b, capacity, dtype, pad=1):
    """(whole buffer as integers, store view of `capacity` stacks in its middle, sentinel, stack length)."""
    stack = 96 * 96 * b.C
    it, fill = (torch.int32, 0x5A5A5A5A) if dtype == torch.float32 else (torch.int16, 0x5A5A)
    buf = torch.full(((capacity + 2 * pad) * stack,), fill, dtype=it, device=b.device)
    store = buf[pad * stack:(pad + capacity) * stack].view(dtype).view(b.out_shape(capacity))
    assert store.data_ptr() % 16 == 0 and store.is_contiguous()
    return buf, store, fill, stack


def check_rows(buf, stack, fill, capacity, rows, pad=1):
    """Row r of the store equals rows[r] for the named rows; every other row, and the bytes before and
    after the store, hold the sentinel."""
    host = buf.cpu().numpy()
    assert (host[:pad * stack] == fill).all() and (host[(pad + capacity) * stack:] == fill).all()
    for r in range(capacity):
        got = host[(pad + r) * stack:(pad + r + 1) * stack]
        if r in rows:
            assert np.array_equal(got, rows[r].reshape(-1)), 'row %d' % r
        else:
            assert (got == fill).all(), 'row %d was written' % r


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('layout', LAYOUTS)
def test_placement(S, layout, dtype):
    _lib, batch, context, vector_env = S
    scene, agents = golden(SPATIAL)
    b = batch.StateBatch([scene], agents=agents, layout=layout)
    assert b.N == 4 and b.C == 7
    f32 = b.render()
    torch.cuda.synchronize()
    assert float(f32.abs().max()) > 0
    want = cast(f32, dtype)
    buf, store, fill, stack = sentinel_store(b, 7, dtype)
    dest = torch.tensor([5, -1, 0, 3], dtype=torch.int64, device=b.device)
    assert b.render_into(store, dest) is store
    torch.cuda.synchronize()
    check_rows(buf, stack, fill, 7, {5: want[0], 0: want[2], 3: want[3]})
    # a host-chosen subset, each of its agents at its own row
    buf, store, fill, stack = sentinel_store(b, 7, dtype)
    b.render_into(store, torch.tensor([6, 1], dtype=torch.int64, device=b.device), slots=[3, 0])
    torch.cuda.synchronize()
    check_rows(buf, stack, fill, 7, {6: want[3], 1: want[0]})
    # the host form of dest gives the same
    buf, store, fill, stack = sentinel_store(b, 7, dtype)
    b.render_into(store, [5, -1, 0, 3])
    torch.cuda.synchronize()
    check_rows(buf, stack, fill, 7, {5: want[0], 0: want[2], 3: want[3]})
    assert _lib.lib.simaps_fault_status(0) == 0


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_all_skipped(S, dtype):
    _lib, batch, context, vector_env = S
    scene, agents = golden(SPATIAL)
    b = batch.StateBatch([scene], agents=agents)
    buf, store, fill, stack = sentinel_store(b, 3, dtype)
    dbg = {k: v.fill_(0x3C) for k, v in b.alloc_debug().items()}
    b.render_into(store, torch.full((4,), -1, dtype=torch.int64, device=b.device), debug=dbg)
    torch.cuda.synchronize()
    check_rows(buf, stack, fill, 3, {})
    for k, v in dbg.items():
        assert (v == 0x3C).all(), k
    assert _lib.lib.simaps_fault_status(0) == 0


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_bad_destinations_are_reported_and_write_nothing(S, dtype):
    """Rows outside [0, capacity) are descriptors the kernel refuses: a fault in the calling context
    under the new kernel id, nothing written for them, the good agent rendered."""
    _lib, batch, context, vector_env = S
    scene, agents = golden(SPATIAL)
    ctx, other = context.Context(), context.Context()
    try:
        b = batch.StateBatch([scene], agents=agents, context=ctx)
        f32 = b.render()
        torch.cuda.synchronize()
        want = cast(f32, dtype)
        capacity = 4
        buf, store, fill, stack = sentinel_store(b, capacity, dtype)
        dest = torch.tensor([1, capacity, -2, 2 ** 40], dtype=torch.int64, device=b.device)
        b.render_into(store, dest)
        torch.cuda.synchronize()
        bits, kernel, unit = ctx.fault_info()
        assert bits == _lib.FAULT_DESCRIPTOR and kernel == 'get_state_into' and unit in (1, 2, 3)
        assert _lib.K_NAMES[13] == 'get_state_into'
        assert other.fault_info() == (0, None, None) and _lib.lib.simaps_fault_status(0) == 0
        check_rows(buf, stack, fill, capacity, {1: want[0]})
        with pytest.raises(_lib.DeviceFault, match='get_state_into'):    # the context's next call, once
            b.render()
        again = b.render()
        torch.cuda.synchronize()
        assert np.array_equal(ints(again), ints(f32))
        assert ctx.fault_info() == (0, None, None)
    finally:
        torch.cuda.synchronize()
        for c in (ctx, other):
            c.fault_status(clear=True)
            c.close()


def _get_state_into(S, ctx, b, R, E, A, P, store, dest, dbg=None):
    _lib = S[0]
    return _lib.call(ctx, 'get_state_into', b.cfg, b.N, _lib.ptr(A), _lib.ptr(E), _lib.ptr(R), _lib.ptr(P),
                     _lib.ptr(b.occupancy), _lib.ptr(b.overhead), _lib.ptr(store), _lib.state_dtype_id(store.dtype),
                     store.shape[0], _lib.ptr(dest), 0, dbg, _lib.stream_handle())


def test_clamped_descriptor_keeps_its_containment(S):
    """A robot index >= num_robots (the clamped-descriptor case of tests/test_gpu_ctx.py: the kernel
    clamps, finishes normally and reports) through simaps_get_state_into and a Context: the fault goes
    under SIMAPS_K_GET_STATE_INTO with that agent's index, in that context only; the others' rows are exact."""
    _lib, batch, context, vector_env = S
    scene, agents = golden(CFG)
    b = batch.StateBatch([scene], agents=agents)
    assert b.N == 4
    want = b.render()
    robots, envs, ag, paths = batch.pack_descriptors([scene], b.agents)
    robots = np.concatenate([robots, np.repeat(robots[:1], 8)])       # records past num_robots exist
    paths = np.concatenate([paths, np.repeat(paths[:1], 40, 0)])
    bad = 2
    ag['robot'][bad] = 6
    dev = lambda x: batch._to_dev(x, b.device)  # noqa: E731
    R, E, A, P = dev(robots), dev(envs), dev(ag), torch.from_numpy(paths).to(b.device)
    rows = [4, 0, 2, 5]
    dest = torch.tensor(rows, dtype=torch.int64, device=b.device)
    a, other = context.Context(), context.Context()
    try:
        for dtype in DTYPES:
            store = b.alloc_store(6, dtype=dtype)
            assert _get_state_into(S, a, b, R, E, A, P, store, dest) == 0
            torch.cuda.synchronize()
            assert a.fault_info() == (_lib.FAULT_DESCRIPTOR, 'get_state_into', bad)
            assert other.fault_info() == (0, None, None) and _lib.lib.simaps_fault_status(0) == 0
            assert a.fault_info(clear=True)[0] == _lib.FAULT_DESCRIPTOR
            got, ref = ints(store), cast(want, dtype)
            for n in range(b.N):
                if n != bad:
                    assert np.array_equal(got[rows[n]], ref[n]), (dtype, n)
    finally:
        torch.cuda.synchronize()
        for c in (a, other):
            c.fault_status(clear=True)
            c.close()


def test_store_beyond_4_gib(S):
    """A float32 store whose last stack begins past 2^32 bytes: the row offset is 64-bit."""
    _lib, batch, context, vector_env = S
    scene, agents = golden(ALL)
    b = batch.StateBatch([scene], agents=agents)
    assert b.C == 10 and b.N == 4
    stack_bytes = 96 * 96 * 10 * 4
    capacity = 11652
    # the smallest store whose last stack begins past 2^32 bytes; the row before it straddles the boundary
    assert stack_bytes == 368640 and (capacity - 2) * stack_bytes < 2 ** 32 < (capacity - 1) * stack_bytes
    f32 = b.render()
    store = b.alloc_store(capacity)                                  # 4.3 GB, never filled
    keep = [0, 1, 11649]
    for r in keep:
        store[r].fill_(-7.25)
    dest = torch.tensor([11650, -1, -1, 11651], dtype=torch.int64, device=b.device)
    b.render_into(store, dest)
    torch.cuda.synchronize()
    assert np.array_equal(ints(store[11650]), ints(f32[0]))
    assert np.array_equal(ints(store[11651]), ints(f32[3]))
    for r in keep:
        assert bool((store[r] == -7.25).all()), r
    assert _lib.lib.simaps_fault_status(0) == 0
    del store


def _bytes(t):
    return t.contiguous().view(torch.uint8).cpu().numpy()


def test_side_outputs(S):
    """Debug cspace / sources / dist / status rows of stored agents: bitwise those of the float32
    render(debug=); a skipped agent's rows keep their fill."""
    _lib, batch, context, vector_env = S
    scene, agents = golden(CFG)
    b = batch.StateBatch([scene], agents=agents)
    ref = {k: torch.zeros_like(v) for k, v in b.alloc_debug().items()}
    f32 = b.render(debug=ref)
    torch.cuda.synchronize()
    assert _bytes(ref['cspace']).any() and _bytes(ref['dist']).any()
    skipped = 1
    for dtype in DTYPES:
        dbg = {k: v.fill_(0x3C) for k, v in b.alloc_debug().items()}
        store = b.alloc_store(5, dtype=dtype)
        b.render_into(store, [2, -1, 0, 4], debug=dbg)
        torch.cuda.synchronize()
        assert np.array_equal(ints(store[2]), cast(f32, dtype)[0])
        for k in ('cspace', 'sources', 'dist', 'status'):
            for n in range(b.N):
                if n == skipped:
                    assert (dbg[k][n] == 0x3C).all(), (dtype, k)
                else:
                    assert np.array_equal(_bytes(dbg[k][n:n + 1]), _bytes(ref[k][n:n + 1])), (dtype, k, n)
    assert _lib.lib.simaps_fault_status(0) == 0


def test_graph_capture_with_a_moving_subset(S):
    """One captured render_into serves steps whose awaiting robots differ: `dest` is device data."""
    _lib, batch, context, vector_env = S
    scene, agents = golden(CFG)
    b = batch.StateBatch([scene], agents=agents)
    b.set_descriptor_arrays(**batch.descriptor_arrays([scene]))       # fixed-size device descriptors
    dtype = torch.bfloat16
    first = cast(b.render(), dtype)
    buf, store, fill, stack = sentinel_store(b, 8, dtype)
    dest = torch.tensor([3, -1, 6, -1], dtype=torch.int64, device=b.device)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        b.render_into(store, dest)
    g.replay()
    torch.cuda.synchronize()
    check_rows(buf, stack, fill, 8, {3: first[0], 6: first[2]})
    # the next step: other robots act, at other rows; its descriptors written in place into the
    # buffers the captured launch reads
    dest.copy_(torch.tensor([-1, 0, 7, 5], dtype=torch.int64))
    rob, pth = b.robots_d, b.paths_d
    b.set_descriptor_arrays(**batch.descriptor_arrays([_moved(scene)]))
    assert rob.shape == b.robots_d.shape and pth.shape == b.paths_d.shape
    rob.copy_(b.robots_d)
    pth.copy_(b.paths_d)
    eager = cast(b.render(), dtype)
    torch.cuda.synchronize()
    assert not np.array_equal(eager, first)
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        # rows 3 and 6 are named by the earlier dest only: they keep the earlier step's stacks
        check_rows(buf, stack, fill, 8, {3: first[0], 6: first[2], 0: eager[1], 7: eager[2], 5: eager[3]})
    assert _lib.lib.simaps_fault_status(0) == 0


def test_host_dest_and_store_checks(S):
    """Every refusal is a ValueError before a launch: the store keeps its sentinel, no fault is posted."""
    _lib, batch, context, vector_env = S
    scene, agents = golden(SPATIAL)
    b = batch.StateBatch([scene], agents=agents, layout='chw')
    buf, store, fill, stack = sentinel_store(b, 4, torch.float16)
    for bad in ([0, 1, 1, 2], [3, 3, -1, -1],                         # duplicates
                [0, 1, 2, 4], [0, 1, 2, -2], [2 ** 40, 0, 1, 2],      # out of range
                [0, 1, 2], [0, 1, 2, 3, -1], []):                     # a wrong length
        with pytest.raises(ValueError):
            b.render_into(store, bad)
    with pytest.raises(ValueError):
        b.render_into(store, [0, 1], slots=[0, 1, 2])
    good = [0, 1, 2, 3]
    dev = lambda v, **kw: torch.tensor(v, device=b.device, **kw)  # noqa: E731
    for bad in (dev(good, dtype=torch.int32), dev(good[:3], dtype=torch.int64), torch.tensor(good, dtype=torch.int64),
                dev([good, good], dtype=torch.int64), dev(good + good, dtype=torch.int64)[::2]):
        with pytest.raises(ValueError):
            b.render_into(store, bad)
    shape = b.out_shape(4)
    for bad in (torch.empty(b.out_shape(4)[1:], dtype=torch.float16, device=b.device),           # no capacity dim
                torch.empty((4, 96, 96, b.C), dtype=torch.float16, device=b.device),             # the other layout
                torch.empty((4, b.C + 1, 96, 96), dtype=torch.float16, device=b.device),         # another C
                torch.empty(shape, dtype=torch.float64, device=b.device),                        # dtype
                torch.empty(shape, dtype=torch.int16, device=b.device),
                torch.empty(shape, dtype=torch.float16),                                         # device
                torch.empty((8,) + shape[1:], dtype=torch.float16, device=b.device)[::2],        # not contiguous
                None):
        with pytest.raises(ValueError):
            b.render_into(bad, good)
    with pytest.raises(ValueError):
        b.alloc_store(4, dtype=torch.float64)
    with pytest.raises(ValueError):
        b.alloc_store(-1)
    for dtype in DTYPES:
        st = b.alloc_store(3, dtype=dtype)
        assert tuple(st.shape) == (3, b.C, 96, 96) and st.dtype == dtype and st.device == b.device
    hwc = batch.StateBatch([scene], agents=agents, layout='hwc')
    assert tuple(hwc.alloc_store(2).shape) == (2, 96, 96, hwc.C) and hwc.alloc_store(2).dtype == torch.float32
    torch.cuda.synchronize()
    check_rows(buf, stack, fill, 4, {})
    assert _lib.lib.simaps_fault_status(0) == 0


def test_vector_env_get_state_into(S):
    """Two steps into one fp16 store at disjoint rows, by an object whose own dtype is float32: after
    the second step the first step's rows are still the first step's states.  Both dest forms."""
    _lib, batch, context, vector_env = S
    scene, _ = golden(CFG)
    steps = [scene, _moved(scene)]
    dtype = torch.float16
    v = vector_env.VectorEnvObservations([scene])
    assert v.dtype == torch.float32 and v.batch.N == 4
    want = []
    for s in steps:
        v.update(scenes=[s])
        want.append(cast(v.batch.render(), dtype))                   # in map-slot order
    torch.cuda.synchronize()
    assert not np.array_equal(want[0], want[1])
    v = vector_env.VectorEnvObservations([scene])
    buf, store, fill, stack = sentinel_store(v.batch, 9, dtype)
    slot = [v.slot[(0, a)] for a in range(4)]
    # step 0: a device tensor in map-slot order, robot 2 not acting
    d0 = torch.full((4,), -1, dtype=torch.int64)
    for a, row in ((0, 0), (1, 1), (3, 2)):
        d0[slot[a]] = row
    assert v.get_state_into(store, d0.to(v.batch.device)) is store
    # step 1: [env][robot] ints, None for "not this robot"
    v.update(scenes=[steps[1]])
    v.get_state_into(store, [[8, None, 5, 4]])
    torch.cuda.synchronize()
    check_rows(buf, stack, fill, 9, {0: want[0][slot[0]], 1: want[0][slot[1]], 2: want[0][slot[3]],
                                     8: want[1][slot[0]], 5: want[1][slot[2]], 4: want[1][slot[3]]})
    for bad in ([[0, 1, 2]], [[0, 1, 2, 3], [4]], [[0, 0, 1, 2]], [[0, 1, 2, 9]], [[0, 1, 2, -1]]):
        with pytest.raises(ValueError):
            v.get_state_into(store, bad)
    assert _lib.lib.simaps_fault_status(0) == 0


@pytest.mark.parametrize('layout', LAYOUTS)
def test_mixed_16_bit(S, layout):
    """MixedStateBatch.render(dtype=d) == render().to(d); float32 through simaps_get_state_mixed_as is
    simaps_get_state_mixed; a configuration index past the table posts its fault and writes nothing."""
    _lib, batch, context, vector_env = S
    from simaps import synthetic
    scenes = [synthetic.make_scene(SPATIAL, 1700), synthetic.make_scene(ALL, 1701)]   # C = 7 and C = 10
    ctx = context.Context()
    try:
        mb = batch.MixedStateBatch(scenes, layout=layout, context=ctx)
        assert len(mb.plan['cfgs']) == 2 and mb.N == 8 and sorted(mb.plan['channels']) == [7, 10]
        f32 = mb.render()
        torch.cuda.synchronize()
        assert f32.dtype == torch.float32 and float(f32.abs().max()) > 0
        for dtype in DTYPES[1:]:
            got = mb.render(dtype=dtype)
            assert got.dtype == dtype and got.shape == f32.shape
            assert np.array_equal(ints(got), cast(f32, dtype)), dtype
            out = mb.alloc_state(dtype=dtype)
            assert mb.render(out=out) is out and np.array_equal(ints(out), cast(f32, dtype))
            views = mb.states(out)
            assert all(v.dtype == dtype for v in views) and len(views) == mb.N
            assert np.array_equal(ints(views[5]), cast(mb.states(f32)[5], dtype))
        with pytest.raises(ValueError):
            mb.render(dtype=torch.float64)
        with pytest.raises(ValueError):
            mb.alloc_state(dtype=torch.int16)
        with pytest.raises(ValueError):
            mb.render(out=mb.alloc_state(dtype=torch.float16), dtype=torch.bfloat16)
        with pytest.raises(ValueError):
            mb.render(out=torch.empty(mb.plan['out_numel'], dtype=torch.int16, device=mb.device))
        # float32 through the new entry point: byte-equal to simaps_get_state_mixed
        out = torch.full_like(f32, float('nan'))
        _lib.check(_lib.call(ctx, 'get_state_mixed_as', mb._cfgs, mb._nrs.ctypes.data, len(mb.plan['cfgs']), mb.N,
                             _lib.ptr(mb.agents_d), _lib.ptr(mb.agent_cfg_d), _lib.ptr(mb.envs_d), _lib.ptr(mb.robots_d),
                             _lib.ptr(mb.paths_d), _lib.ptr(mb.occupancy), _lib.ptr(mb.map_off_d), _lib.ptr(mb.overhead),
                             _lib.ptr(out), _lib.ptr(mb.out_off_d), _lib.STATE_F32, _lib.stream_handle()))
        torch.cuda.synchronize()
        assert np.array_equal(_bytes(out), _bytes(f32))
        assert ctx.fault_info() == (0, None, None)
        # agent 0's configuration index past the table, in 16-bit
        mb.agent_cfg_d[0] = 99
        for dtype in DTYPES[1:]:
            out = torch.full((mb.plan['out_numel'],), 0x5A5A, dtype=torch.int16, device=mb.device).view(dtype)
            mb.render(out=out)
            torch.cuda.synchronize()
            assert ctx.fault_info(clear=True) == (_lib.FAULT_DESCRIPTOR, 'get_state_mixed', 0)
            got, ref = mb.states(out), mb.states(f32)
            assert (ints(got[0]) == 0x5A5A).all()
            for n in range(1, mb.N):
                assert np.array_equal(ints(got[n]), cast(ref[n], dtype)), (dtype, n)
        assert _lib.lib.simaps_fault_status(0) == 0
    finally:
        torch.cuda.synchronize()
        ctx.fault_status(clear=True)
        ctx.close()
