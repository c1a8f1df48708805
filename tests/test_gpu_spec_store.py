"""GPU: the compile-time get_state instances of the store launches and the 16-bit launches
(include/simaps_spec_store.h, csrc/simaps_spec_store.inc) against the generic kernel of the same build.

A render_into() / render(dtype=) without debug buffers of a standard stack launches an instance (the
query says which); the same call with a debug `status` buffer is the entry point's generic kernel.
The two results must be equal bit for bit (integer views), the rows of the store that `dest` does not
name must keep their sentinel, and every fault must carry the same word, kernel id and unit.

One env (4 agents) per configuration; the near-wall case renders 32 stacks.  FAMILIES
(tests/test_spec_store_abi.py) says which launch families the library dispatches to instances: a
family left generic is still compared here (generic against generic), with the query expecting 0.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from test_spec_store_abi import FAMILIES

pytestmark = pytest.mark.gpu

FLAGSHIP = 'lifting_4-small_divider'
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ['f32', 'bf16', 'f16']
# configuration, instance, room class: S1 + small-room twin (1-cell column sweeps); S1 without a room
# class (2-cell sweeps, the other tile layout); S2 (one source, 12 render waves) + small-room twin
CASES = [(FLAGSHIP, 1, 1), ('pushing_4-large_empty', 1, 0), ('rescue_4-small_empty', 2, 1)]
CAPACITY = 9
DEST = [7, -1, 0, 3]


@pytest.fixture(scope='module')
def S():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a GPU (run with -m gpu on an MI355X)')
    from simaps import _lib, batch, context, synthetic
    _lib.lib.simaps_fault_status(1)
    yield _lib, batch, context, synthetic
    _lib.lib.simaps_fault_status(1)


_BATCH = {}


def one_env(S, name):
    """The StateBatch of env 0 of a configuration and its float32 instance render, made once."""
    if name not in _BATCH:
        _lib, batch, context, synthetic = S
        scene = synthetic.make_scene(name, 0)
        b = batch.StateBatch([scene])
        assert b.N == 4 and bool(b.cfg.layout_chw)
        f32 = b.render()
        torch.cuda.synchronize()
        _BATCH[name] = (scene, b, f32)
    return _BATCH[name]


def ints(t):
    """The integer view of a float32 / bf16 / fp16 tensor, on the host."""
    t = t.detach().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu().numpy()


def sentinel_store(b, capacity, dtype):
    """(the store, its sentinel): every element's bits 0x5A5A / 0x5A5A5A5A."""
    it, fill = (torch.int32, 0x5A5A5A5A) if dtype == torch.float32 else (torch.int16, 0x5A5A)
    buf = torch.full((capacity * 96 * 96 * b.C,), fill, dtype=it, device=b.device)
    return buf.view(dtype).view(b.out_shape(capacity)), fill


def status_dbg(b, n=None):
    """A debug dict with a status buffer only: what selects the generic kernel."""
    return {'status': torch.zeros(b.N if n is None else n, dtype=torch.int32, device=b.device)}


def expect(S, b, dtype, into, inst, room):
    """The queries' answers for the launch: (inst, room) where its family is dispatched, generic
    otherwise; always generic with a debug output."""
    _lib = S[0]
    on = FAMILIES['into' if into else 'plain16'] or (dtype == torch.float32 and not into)
    want = (inst, room) if on else (_lib.SPEC_GENERIC, _lib.ROOM_NONE)
    assert (b.kernel_instance(dtype=dtype, into=into), b.room_class(dtype=dtype, into=into)) == want
    assert b.kernel_instance(debug=True, dtype=dtype, into=into) == _lib.SPEC_GENERIC
    assert b.room_class(debug=True, dtype=dtype, into=into) == _lib.ROOM_NONE


def into_both(S, b, dtype, dest, capacity=CAPACITY, slots=None, debug=None):
    """(instance store, generic store, sentinel) of render_into with the same device `dest`."""
    n = b.N if slots is None else len(slots)
    dest = dest if isinstance(dest, torch.Tensor) else torch.tensor(dest, dtype=torch.int64, device=b.device)
    spec, fill = sentinel_store(b, capacity, dtype)
    gen, _ = sentinel_store(b, capacity, dtype)
    assert b.render_into(spec, dest, slots=slots) is spec
    b.render_into(gen, dest, slots=slots, debug=debug if debug is not None else status_dbg(b, n))
    torch.cuda.synchronize()
    return spec, gen, fill


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('name, inst, room', CASES)
def test_store_instance_equals_generic(S, name, inst, room, dtype):
    _lib = S[0]
    scene, b, f32 = one_env(S, name)
    expect(S, b, dtype, True, inst, room)
    spec, gen, fill = into_both(S, b, dtype, DEST)
    got, ref = ints(spec), ints(gen)
    assert np.array_equal(got, ref)                                     # the whole store
    for r in range(CAPACITY):
        if r not in DEST:
            assert (got[r] == fill).all(), 'row %d was written' % r
    want = ints(f32.cpu().to(dtype))
    for n, r in enumerate(DEST):
        if r >= 0:
            assert np.array_equal(got[r], want[n]), (n, r)              # and each row is render()'s stack
    assert float(f32.abs().max()) > 0 and not torch.isnan(f32).any()
    assert _lib.lib.simaps_fault_status(0) == 0


@pytest.mark.parametrize('dtype', DTYPES[1:], ids=IDS[1:])
@pytest.mark.parametrize('name, inst, room', CASES)
def test_plain_16_bit_instance_equals_generic(S, name, inst, room, dtype):
    _lib = S[0]
    scene, b, f32 = one_env(S, name)
    expect(S, b, dtype, False, inst, room)
    spec = b.render(dtype=dtype)
    gen = b.render(dtype=dtype, debug=status_dbg(b))
    torch.cuda.synchronize()
    assert spec.dtype == dtype and tuple(spec.shape) == b.out_shape(b.N)
    assert np.array_equal(ints(spec), ints(gen))
    assert np.array_equal(ints(spec), ints(f32.cpu().to(dtype)))         # the float32 instance, cast
    assert _lib.lib.simaps_fault_status(0) == 0


def test_flagship_float32_store_equals_the_oracle(S):
    import oracle
    scene, b, f32 = one_env(S, FLAGSHIP)
    store, fill = sentinel_store(b, CAPACITY, torch.float32)
    dest = [5, 2, 8, 0]
    b.render_into(store, dest)
    torch.cuda.synchronize()
    hwc = b.as_hwc(store).cpu().numpy()
    for n, (e, a) in enumerate(b.agents):
        ref = oracle.AgentOracle(scene, a).get_state()
        assert np.array_equal(hwc[dest[n]].view(np.int32), ref.view(np.int32)), 'agent %d' % a


def _near_walls(scene, seed):
    """The recipe of tests/test_gpu_spec.py: robots 2 and 3 moved anywhere in the room up to 2 cm from
    its edge, so that shortest-path sources are snapped to the closest free cell."""
    rs = np.random.RandomState(seed)
    rl, rw = scene['room_length'], scene['room_width']
    for r in scene['robots'][2:]:
        r['position'] = (float(rs.uniform(-rl / 2 + 0.02, rl / 2 - 0.02)),
                         float(rs.uniform(-rw / 2 + 0.02, rw / 2 - 0.02)), 0)
        r['waypoint_positions'] = [r['position']] + list(r['waypoint_positions'][1:])
    return scene


def test_near_walls_32_stacks_into_a_bf16_store(S):
    """8 seeded envs of the flagship (32 stacks), two robots of each next to walls, into a bf16 store of
    40 rows at shuffled rows, 5 agents skipped: among the rendered stacks some converge in 3 and some
    in 4 SSSP rounds and some sources are snapped (read from the generic run's debug outputs)."""
    _lib, batch, context, synthetic = S
    b = batch.StateBatch([_near_walls(synthetic.make_scene(FLAGSHIP, 100 + e), 100 + e) for e in range(8)])
    assert b.N == 32
    expect(S, b, torch.bfloat16, True, 1, 1)
    rs = np.random.RandomState(4)
    rows = rs.permutation(40)[:32].astype(np.int64)
    skipped = sorted(int(k) for k in rs.permutation(32)[:5])
    rows[skipped] = -1
    dbg = {k: v.zero_() for k, v in b.alloc_debug().items()}
    spec, gen, fill = into_both(S, b, torch.bfloat16, [int(r) for r in rows], capacity=40, debug=dbg)
    got = ints(spec)
    assert np.array_equal(got, ints(gen))
    named = set(int(r) for r in rows if r >= 0)
    assert len(named) == 27
    for r in range(40):
        assert (got[r] == fill).all() == (r not in named), r
    keep = rows >= 0
    st = dbg['status'].cpu().numpy()[keep]
    src = dbg['sources'].cpu().numpy()[keep]
    rounds, snapped = set((st >> 8).tolist()), int((src[:, :, :2] != src[:, :, 2:]).any(2).sum())
    print('rounds per rendered stack:', sorted(rounds), 'snapped sources:', snapped)
    assert {3, 4} <= rounds and snapped > 0                              # what this case is there to cover
    assert ((st & 14) == 0).all()                                        # no round cap, timeout or clamp
    assert (dbg['status'].cpu().numpy()[~keep] == 0).all()               # a skipped agent's debug row: untouched
    assert _lib.lib.simaps_fault_status(0) == 0


def _fault(ctx):
    """(bits, kernel id, unit, named info) of the context's fault word, cleared."""
    k, u = ctypes.c_int(-2), ctypes.c_int(-2)
    from simaps import _lib
    bits = _lib.lib.simaps_ctx_fault_info(ctx.handle, 0, ctypes.byref(k), ctypes.byref(u))
    return bits, k.value, u.value, ctx.fault_info(clear=True)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_bad_rows_post_the_same_fault_and_write_nothing(S, dtype):
    """A dest value equal to capacity, a dest value of -2 (one per launch, so that the posting unit is
    determined), and all of dest at -1: instance against generic kernel."""
    _lib, batch, context, synthetic = S
    scene = one_env(S, FLAGSHIP)[0]
    ctx = context.Context()
    try:
        b = batch.StateBatch([scene], context=ctx)
        expect(S, b, dtype, True, 1, 1)
        want = ints(one_env(S, FLAGSHIP)[2].cpu().to(dtype))
        for dest, unit in (([1, CAPACITY, -1, 2], 1), ([1, -1, -2, 2], 2), ([-1, -1, -1, -1], None)):
            d = torch.tensor(dest, dtype=torch.int64, device=b.device)
            got = []
            for dbg in (None, status_dbg(b)):                            # the instance, then the generic kernel
                store, fill = sentinel_store(b, CAPACITY, dtype)
                b.render_into(store, d, debug=dbg)
                torch.cuda.synchronize()
                got.append((_fault(ctx), ints(store)))
            (f1, s1), (f2, s2) = got
            assert f1 == f2, dest
            if unit is None:
                assert f1[0] == 0 and f1[3] == (0, None, None), f1
                assert (s1 == fill).all() and (s2 == fill).all()
            else:
                assert f1 == (_lib.FAULT_DESCRIPTOR, 13, unit, (_lib.FAULT_DESCRIPTOR, 'get_state_into', unit)), f1
                assert np.array_equal(s1, s2)
                for r in range(CAPACITY):
                    if r == 1:
                        assert np.array_equal(s1[r], want[0])
                    elif r == 2:
                        assert np.array_equal(s1[r], want[3])
                    else:
                        assert (s1[r] == fill).all(), r
        assert _lib.lib.simaps_fault_status(0) == 0
    finally:
        torch.cuda.synchronize()
        ctx.fault_status(clear=True)
        ctx.close()


def test_descriptor_clamp_posts_the_same_fault_through_an_instance(S):
    """An agent's robot index past num_robots (the recipe of tests/test_gpu_spec.py): the kernel clamps
    it, finishes normally and posts SIMAPS_FAULT_DESCRIPTOR with `where` = (the entry point's kernel,
    the agent) -- get_state_into for the store launches, get_state for the plain 16-bit ones, which
    share their instances' kernels with them."""
    _lib, batch, context, synthetic = S
    b = batch.StateBatch([synthetic.make_scene(FLAGSHIP, 7 + e) for e in range(2)])
    robots, envs, ag, paths = batch.pack_descriptors(b.scenes, b.agents)
    robots = np.concatenate([robots, np.repeat(robots[:1], 8)])
    paths = np.concatenate([paths, np.repeat(paths[:1], 40, 0)])
    ag['robot'][5] = 6                                                   # 8 agents, only agent 5 is bad
    R, E, A = (batch._to_dev(x, b.device) for x in (robots, envs, ag))
    P = torch.from_numpy(paths).to(b.device)
    dest = torch.tensor([3, 9, 0, 7, 1, 4, 8, 6], dtype=torch.int64, device=b.device)
    ctx = context.Context()
    common = (b.cfg, b.N, _lib.ptr(A), _lib.ptr(E), _lib.ptr(R), _lib.ptr(P), _lib.ptr(b.occupancy), _lib.ptr(b.overhead))
    try:
        for dtype, into in [(torch.float32, True), (torch.bfloat16, True), (torch.float16, True),
                            (torch.bfloat16, False), (torch.float16, False)]:
            expect(S, b, dtype, into, 1, 1)
            got = []
            for generic in (False, True):
                status = torch.zeros(b.N, dtype=torch.int32, device=b.device)
                d = _lib.Debug(None, None, None, status.data_ptr(), None) if generic else None
                out, fill = sentinel_store(b, 10 if into else b.N, dtype)
                did = _lib.state_dtype_id(dtype)
                if into:
                    rc = _lib.call(ctx, 'get_state_into', *common, _lib.ptr(out), did, 10, _lib.ptr(dest), 0, d,
                                   _lib.stream_handle())
                else:
                    rc = _lib.call(ctx, 'get_state_as', *common, _lib.ptr(out), did, 0, d, _lib.stream_handle())
                assert rc == 0
                torch.cuda.synchronize()
                got.append((_fault(ctx), ints(out)))
                if generic:
                    st = status.cpu().numpy()
                    assert st[5] & 8 and not (st[[0, 1, 2, 3, 4, 6, 7]] & 8).any()
            (f1, o1), (f2, o2) = got
            kid, kname = (13, 'get_state_into') if into else (1, 'get_state')
            assert f1 == f2 == (_lib.FAULT_DESCRIPTOR, kid, 5, (_lib.FAULT_DESCRIPTOR, kname, 5)), (dtype, into, f1, f2)
            assert np.array_equal(o1, o2), (dtype, into)
            assert (o1[2] == fill).all() == into                        # row 2 of the store is nobody's
    finally:
        torch.cuda.synchronize()
        ctx.fault_status(clear=True)
        ctx.close()


def test_graph_capture_follows_a_rewritten_dest(S):
    """One captured instance render_into, replayed twice with `dest` rewritten on the device in
    between: each replay equals the eager generic launch for that dest."""
    _lib, batch, context, synthetic = S
    scene, b, f32 = one_env(S, FLAGSHIP)
    dtype = torch.bfloat16
    expect(S, b, dtype, True, 1, 1)
    dests = [torch.tensor(v, dtype=torch.int64, device=b.device) for v in ([3, -1, 6, -1], [-1, 0, 7, 5])]
    dest = dests[0].clone()
    store, fill = sentinel_store(b, CAPACITY, dtype)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        b.render_into(store, dest)
    for want in dests:
        store.view(torch.int16).fill_(fill)
        dest.copy_(want)                                                 # a device-to-device rewrite
        g.replay()
        gen, _ = sentinel_store(b, CAPACITY, dtype)
        b.render_into(gen, want, debug=status_dbg(b))
        torch.cuda.synchronize()
        got = ints(store)
        assert np.array_equal(got, ints(gen)), want.tolist()
        assert sorted(r for r in range(CAPACITY) if not (got[r] == fill).all()) == sorted(v for v in want.tolist() if v >= 0)
    assert _lib.lib.simaps_fault_status(0) == 0


def _xy(b, row, col):
    c = b.cfg
    return (float((c.room_j0 + col + 0.5 - b.W / 2) / 96.0), float((b.H / 2 - (c.room_i0 + row + 0.5)) / 96.0), 0)


def _with_paths(b, scene, rows):
    """Every robot of the scene active, at row rows[0] with an intention path over a waypoint to a
    target at row rows[1] (the recipe of tests/test_gpu_sweepdiet.py)."""
    for k, r in enumerate(scene['robots']):
        c = 10 + 22 * k
        r['position'] = _xy(b, rows[0], c)
        r['waypoint_positions'] = [r['position'], _xy(b, (rows[0] + rows[1]) // 2, c + 6), _xy(b, rows[1], c + 3)]
        r['waypoint_index'] = 1
        r['target_ee'] = _xy(b, rows[1], c + 8)
        r['idle'] = False


def test_late_scratch_path_through_the_bf16_store_instance(S):
    """The late path of zero_scratch_early (every render wave of the two-source instance finds the
    sweep track's scratch still held: the diagnostic ring build) through the bf16 store instance S1:
    env 0 has intention segments in the tile rows that alias the scratch, env 1 has none there.
    Against the generic kernel of that library and against the product's stacks."""
    _lib, batch, context, synthetic = S
    scenes = [synthetic.make_scene(FLAGSHIP, 21), synthetic.make_scene(FLAGSHIP, 22)]
    b = batch.StateBatch(scenes)
    _with_paths(b, scenes[0], (38, 6))
    _with_paths(b, scenes[1], (22, 26))
    b.set_descriptors(scenes)
    c = b.cfg
    occ = []
    for sc in scenes:
        o = np.array(sc['occupancy'][0], dtype=np.uint8)
        o[c.room_i0:c.room_i0 + c.room_h, c.room_j0:c.room_j0 + c.room_w] = 0
        occ.append(np.repeat(o[None], 4, 0))
    b.set_maps(occupancy=np.concatenate(occ))
    dtype = torch.bfloat16
    expect(S, b, dtype, True, 1, 1)
    dest = torch.tensor([8, 1, 5, 0, 3, 9, 7, 2], dtype=torch.int64, device=b.device)
    prod, prod_gen, fill = into_both(S, b, dtype, dest, capacity=10)
    assert np.array_equal(ints(prod), ints(prod_gen))
    ch = 4                                                               # overhead, robot, 2 x sp, intention
    f32 = b.render()
    assert f32.shape[1] == 5 and float(f32[:4, ch].abs().max()) > 0 and float(f32[4:, ch].abs().max()) > 0
    lib = os.path.join(os.path.dirname(_lib.__file__), 'libsimaps_diagring.so')
    if not os.path.exists(lib):
        pytest.fail('build the diagnostic library first: make -C spatial-intention-maps_amd/csrc diag')
    L = _lib._load(lib)
    assert L.simaps_fault_status(1) == 0
    assert L.simaps_get_state_instance_as(b.cfg, _lib.STATE_BF16, 1, 0) == b.kernel_instance(dtype=dtype, into=True)
    status = torch.zeros(b.N, dtype=torch.int32, device=b.device)
    outs = []
    for d in (None, _lib.Debug(None, None, None, status.data_ptr(), None)):   # S1 (late path), then generic
        out, _ = sentinel_store(b, 10, dtype)
        assert L.simaps_get_state_into(b.cfg, b.N, _lib.ptr(b.agents_d), _lib.ptr(b.envs_d), _lib.ptr(b.robots_d),
                                       _lib.ptr(b.paths_d), _lib.ptr(b.occupancy), _lib.ptr(b.overhead), _lib.ptr(out),
                                       _lib.STATE_BF16, 10, _lib.ptr(dest), 0, d, _lib.stream_handle()) == 0
        torch.cuda.synchronize()
        outs.append(ints(out))
    assert L.simaps_fault_status(0) == 0 and ((status.cpu().numpy() & 14) == 0).all()
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], ints(prod))
    assert (outs[0][4] == fill).all() and (outs[0][6] == fill).all()     # the two rows dest does not name


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('kind', ['hwc', 'history'])
def test_other_stacks_keep_the_generic_kernel(S, kind, dtype):
    """An HWC store and a -history configuration: generic per the queries, and what they gave --
    render()'s stacks in that dtype at the named rows, the sentinel elsewhere."""
    _lib, batch, context, synthetic = S
    name = FLAGSHIP + ('-history' if kind == 'history' else '')
    b = batch.StateBatch([synthetic.make_scene(name, 0)], layout='hwc' if kind == 'hwc' else 'chw')
    for into in (False, True):
        assert b.kernel_instance(dtype=dtype, into=into) == _lib.SPEC_GENERIC
        assert b.room_class(dtype=dtype, into=into) == _lib.ROOM_NONE
    f32 = b.render()
    torch.cuda.synchronize()
    want = ints(f32.cpu().to(dtype))
    plain, gen, fill = into_both(S, b, dtype, DEST)
    got = ints(plain)
    assert np.array_equal(got, ints(gen))
    for r in range(CAPACITY):
        if r in DEST:
            assert np.array_equal(got[r], want[DEST.index(r)]), r
        else:
            assert (got[r] == fill).all(), r
    if dtype != torch.float32:
        assert np.array_equal(ints(b.render(dtype=dtype)), want)
    assert _lib.lib.simaps_fault_status(0) == 0
