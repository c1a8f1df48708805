"""GPU tests of the context-scoped C ABI (include/simaps_ctx.h) and simaps.context.Context.

A context owns its fault record, path mode and scratch pool.  The twins are bitwise the old entry
points; a fault posted through one context is invisible to every other and says which kernel and
which unit of the batch posted it; contexts work from several threads and on a second device.

A "device fault" here is the status bit of a descriptor clamp (the recipe of
tests/test_gpu_faults.py::test_descriptor_clamp_is_reported): the kernel clamps a robot index past
num_robots, finishes normally and reports it.  Only the product library is used.
"""
import ctypes
import threading

import numpy as np
import pytest
import torch

import goldens as G
import oracle as O

pytestmark = pytest.mark.gpu

CFG = 'lifting_4-small_divider'


@pytest.fixture(scope='module')
def S():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a GPU (run with -m gpu on an MI355X)')
    from simaps import _lib, batch, context, synthetic
    _lib.lib.simaps_fault_status(1)
    yield _lib, batch, context, synthetic
    _lib.lib.simaps_fault_status(1)


@pytest.fixture
def AB(S):
    """Two created contexts; every record touched is cleared and both are destroyed afterwards."""
    _lib, batch, context, synthetic = S
    prev = _lib.lib.simaps_path_mode(0)
    a, b = context.Context(), context.Context()
    yield a, b
    torch.cuda.synchronize()
    for c in (a, b):
        if c._open:
            c.fault_status(clear=True)
        c.close()
    _lib.lib.simaps_fault_status(1)
    _lib.lib.simaps_path_mode(prev)


def _i32(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint8 if a.dtype.itemsize == 1 else np.int32)


def _same(x, y):
    x, y = _i32(x), _i32(y)
    return x.shape == y.shape and np.array_equal(x, y)


def _detours(n=4):
    """n path goldens of CFG (scenes of seeds 60, 61), one per agent, whose path is not the straight
    line: (env, robot, source, target, the reference's path)."""
    z = G.load('paths.npz')
    items = {}
    for k in sorted(z.files):
        if k.startswith(CFG + '_e') and k.endswith('_path') and len(z[k]) > 2:
            key = k[:-len('_path')]
            e, a = (int(x) for x in key.rsplit('_q', 1)[0].rsplit('_e', 1)[1].split('_a'))
            items.setdefault((e, a), (e, a, z[key + '_src'], z[key + '_tgt'], z[k]))
    assert len(items) >= n
    return list(items.values())[:n]


def _bad_descriptors(S, scenes, bad_agent):
    """(batch, R, E, A, P): the device descriptors of `scenes` with agent `bad_agent`'s robot index 6
    (>= num_robots 4), the robots / paths arrays padded like test_descriptor_clamp_is_reported."""
    _lib, batch, context, synthetic = S
    b = batch.StateBatch(scenes)
    robots, envs, ag, paths = batch.pack_descriptors(scenes, b.agents)
    robots = np.concatenate([robots, np.repeat(robots[:1], 8)])
    paths = np.concatenate([paths, np.repeat(paths[:1], 40, 0)])
    ag['robot'][bad_agent] = 6
    dev = lambda x: batch._to_dev(x, b.device)  # noqa: E731
    return b, dev(robots), dev(envs), dev(ag), torch.from_numpy(paths).to(b.device)


def _get_state(S, ctx, b, R, E, A, P, out):
    _lib = S[0]
    return _lib.call(ctx, 'get_state', b.cfg, b.N, _lib.ptr(A), _lib.ptr(E), _lib.ptr(R), _lib.ptr(P),
                     _lib.ptr(b.occupancy), _lib.ptr(b.overhead), _lib.ptr(out), 0, None, _lib.stream_handle())


def _run_everything(S, ctx):
    """Every compute entry point once on fixed inputs, through `ctx` (None: the old entry points)."""
    _lib, batch, context, synthetic = S
    from simaps import vector_env
    out = {}
    scenes = [synthetic.make_scene(CFG, e) for e in range(2)]
    b = batch.StateBatch(scenes, context=ctx)
    out['render'] = b.render()                                                      # get_state, 8 stacks
    rs = np.random.RandomState(3)
    tgt = rs.uniform(-0.4, 0.4, size=(b.N, 2, 2))
    out['rec_miss'] = b.receptacle_distances(tgt)                                   # sp_distance
    out['rec_hit'] = b.receptacle_distances(tgt[:, ::-1].copy())                    # sp_lookup
    cs, th = b.build_cspace()                                                       # build_cspace
    out['cspace'], out['thin'] = cs, th
    px = rs.randint(0, min(b.H, b.W), size=(b.N, 3, 2)).astype(np.int32)
    out['snap'] = b.snap_pixels(px)                                                 # snap_sources
    for k, v in b.global_maps().items():                                            # global_maps
        out['global_' + k] = v
    pts = rs.uniform(-0.5, 0.5, size=(b.N, 50, 3)).astype(np.float32)
    seg = np.where(rs.rand(b.N, 50) < 0.5, 0.25, 0.0).astype(np.float32)
    marks = torch.zeros_like(b.occupancy)
    b.scatter_obstacles(pts, seg, 0.25, out=marks)                                  # occupancy_scatter
    out['scatter'] = marks
    frame = synthetic.camera_images(scenes[0], 1, 'forward', seed=11)
    b.ingest(frame[0][None], frame[1][None].astype(np.int32), slots=[1])            # ingest, one frame
    out['ingest_occ'], out['ingest_ovh'] = b.occupancy.clone(), b.overhead.clone()
    items = _detours()                                                              # shortest_path, 4 queries
    pb = batch.StateBatch([synthetic.make_scene(CFG, 60 + e) for e in range(2)], context=ctx)
    paths = pb.shortest_paths(np.stack([i[2] for i in items]), np.stack([i[3] for i in items]),
                              slots=[pb.agents.index((e, a)) for e, a, *_ in items])
    for q, (p, it) in enumerate(zip(paths, items)):
        assert np.array_equal(np.array([w[:2] for w in p]), it[4]), q               # (and the reference's)
        out['path_%d' % q] = np.array(p, dtype=np.float64)
    g = G.load('sssp.npz')                                                          # sssp_grid, grid_path
    gg = vector_env.GridGraph(g['demo_cspace'], context=ctx)
    assert g['demo_cspace'].shape == (232, 232)
    out['sssp'] = gg.shortest_path_image((75, 156))
    assert _same(out['sssp'], g['demo_image'])
    s0 = G.load('paths.npz')
    for q, p in enumerate(gg.shortest_paths([(tuple(s0['demo_%d_src' % q]), tuple(s0['demo_%d_tgt' % q]))
                                             for q in range(3)])):
        out['grid_path_%d' % q] = np.array(p, dtype=np.int32)
    mixed = [dict(synthetic.make_scene(CFG, 20 + e), rotate_rounding=r) for e, r in enumerate(('fma', 'plain'))]
    mb = batch.MixedStateBatch(mixed, context=ctx)                                  # get_state_mixed
    assert len(mb.plan['cfgs']) == 2
    out['mixed'] = mb.render()
    torch.cuda.synchronize()
    return {k: _i32(v) for k, v in out.items()}


def test_twins_are_bitwise_the_old_entry_points(S, AB):
    _lib, batch, context, synthetic = S
    a, _ = AB
    old = _run_everything(S, None)
    new = _run_everything(S, a)
    assert sorted(old) == sorted(new) and len(old) >= 20
    for k in old:
        assert old[k].shape == new[k].shape and np.array_equal(old[k], new[k]), k
    assert a.fault_info() == (0, None, None)
    assert _lib.lib.simaps_fault_status(0) == 0


def test_fault_isolation(S, AB):
    _lib, batch, context, synthetic = S
    a, b = AB
    bt, R, E, A, P = _bad_descriptors(S, [synthetic.make_scene(CFG, 5)], 1)
    out = bt.alloc_state()
    assert _get_state(S, a, bt, R, E, A, P, out) == 0                   # posts FAULT_DESCRIPTOR through a
    torch.cuda.synchronize()
    assert a.fault_status() == _lib.FAULT_DESCRIPTOR
    assert b.fault_status() == 0
    assert _lib.lib.simaps_fault_status(0) == 0
    good = (bt.robots_d, bt.envs_d, bt.agents_d, bt.paths_d)
    assert _get_state(S, b, bt, *good, out) == 0
    assert _get_state(S, None, bt, *good, out) == 0
    assert _get_state(S, a, bt, *good, out) == _lib.EDEVICE            # exactly once, and clears
    msg = _lib.lib.simaps_last_error()
    assert b'descriptor clamped' in msg and msg.endswith(b' in get_state, unit 1')
    assert _get_state(S, a, bt, *good, out) == 0
    torch.cuda.synchronize()
    assert a.fault_status() == 0 and b.fault_status() == 0 and _lib.lib.simaps_fault_status(0) == 0


def test_attribution(S, AB):
    _lib, batch, context, synthetic = S
    a, _ = AB
    FD = _lib.FAULT_DESCRIPTOR
    scenes = [synthetic.make_scene(CFG, 7 + e) for e in range(2)]
    bt, R, E, A, P = _bad_descriptors(S, scenes, 5)                     # 8 agents, only agent 5 is bad
    out = bt.alloc_state()
    st = _lib.stream_handle()
    p = _lib.ptr

    assert _get_state(S, a, bt, R, E, A, P, out) == 0
    torch.cuda.synchronize()
    assert a.fault_info() == (FD, 'get_state', 5)                       # reading does not clear
    assert a.fault_info(clear=True) == (FD, 'get_state', 5)
    assert a.fault_info() == (0, None, None)

    cs = torch.empty((bt.N, bt.H, bt.W), dtype=torch.uint8, device=bt.device)
    assert _lib.call(a, 'build_cspace', bt.cfg, bt.N, p(A), p(E), p(R), p(bt.occupancy), p(cs), None, st) == 0
    torch.cuda.synchronize()
    assert a.fault_info(clear=True) == (FD, 'occupancy_map', 5)         # blockIdx.y, not blockIdx.x

    gm = torch.empty((bt.N, bt.H, bt.W), dtype=torch.float32, device=bt.device)
    assert _lib.call(a, 'global_maps', bt.cfg, bt.N, p(A), p(E), p(R), p(P), p(bt.overhead), p(gm), None, None, None,
                     st) == 0
    torch.cuda.synchronize()
    assert a.fault_info(clear=True) == (FD, 'global_maps', 5)

    mixed = [dict(synthetic.make_scene(CFG, 20 + e), rotate_rounding=r) for e, r in enumerate(('fma', 'plain'))]
    mb = batch.MixedStateBatch(mixed, context=a)
    ac = mb.plan['agent_cfg'].copy()
    ac[3] = len(mb.plan['cfgs'])                                        # a configuration index past the table
    mb.agent_cfg_d = torch.from_numpy(ac).to(mb.device)
    mb.render()
    torch.cuda.synchronize()
    assert a.fault_info() == (FD, 'get_state_mixed', 3)
    with pytest.raises(_lib.DeviceFault, match='in get_state_mixed, unit 3'):
        a.check_faults()

    good = batch.StateBatch(scenes, context=a)
    good.render()
    torch.cuda.synchronize()
    assert a.fault_info() == (0, None, None)                            # a clean render: nothing known

    # the same through the old entry point: the default context's record, read with a NULL context
    assert _get_state(S, None, bt, R, E, A, P, out) == 0
    torch.cuda.synchronize()
    k, u = ctypes.c_int(0), ctypes.c_int(0)
    assert _lib.lib.simaps_ctx_fault_info(None, 0, ctypes.byref(k), ctypes.byref(u)) == FD
    assert (_lib.K_NAMES[k.value], u.value) == ('get_state', 5)
    assert a.fault_info() == (0, None, None)
    assert _lib.lib.simaps_fault_status(1) == FD                        # the old name clears `where` too
    assert _lib.lib.simaps_ctx_fault_info(None, 0, ctypes.byref(k), ctypes.byref(u)) == 0
    assert (k.value, u.value) == (-1, -1)


def test_path_mode_is_per_context(S, AB):
    _lib, batch, context, synthetic = S
    a, b = AB
    assert a.path_mode(1) == 0
    assert b.path_mode(3) == 0
    assert _lib.lib.simaps_path_mode(0) == 0
    assert a.path_mode(0) == 1
    assert a.path_mode(1) == 0
    items = _detours()
    scenes = [synthetic.make_scene(CFG, 60 + e) for e in range(2)]
    got = []
    for c in (a, b):
        pb = batch.StateBatch(scenes, context=c)
        got.append(pb.shortest_paths(np.stack([i[2] for i in items]), np.stack([i[3] for i in items]),
                                     slots=[pb.agents.index((e, x)) for e, x, *_ in items]))
    assert got[0] == got[1]
    for p, it in zip(got[0], items):
        assert len(p) > 2 and np.array_equal(np.array([w[:2] for w in p]), it[4])
    assert (a.path_mode(0), b.path_mode(0)) == (1, 3)


def test_two_threads_two_contexts(S):
    _lib, batch, context, synthetic = S
    seeds = ([100, 101], [200, 201])
    results, errors = [None, None], []

    def worker(k):
        try:
            torch.cuda.set_device(0)
            with context.Context() as c:
                st = torch.cuda.Stream()
                b = batch.StateBatch([synthetic.make_scene(CFG, s) for s in seeds[k]], context=c)
                out = b.alloc_state()
                for _ in range(20):
                    b.render(out=out, stream=st)
                st.synchronize()
                results[k] = (out.cpu().numpy(), c.fault_status())
        except Exception as e:  # noqa: BLE001  (reported by the main thread)
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for k in range(2):
        serial = batch.StateBatch([synthetic.make_scene(CFG, s) for s in seeds[k]]).render().cpu().numpy()
        assert _same(results[k][0], serial), k
        assert results[k][1] == 0
    assert _lib.lib.simaps_fault_status(0) == 0


def test_lifetime(S):
    _lib, batch, context, synthetic = S
    scenes = [synthetic.make_scene(CFG, 30 + e) for e in range(2)]
    c = context.Context()
    b = batch.StateBatch(scenes, context=c)
    side = torch.cuda.Stream()
    out = b.render(stream=side)
    c.close()                                       # destroy synchronises the device: the render is done
    assert _same(out, batch.StateBatch(scenes).render())
    c.close()                                       # a no-op
    with pytest.raises(_lib.SimapsError, match='not a live context'):
        b.render()
    with pytest.raises(_lib.SimapsError):
        c.fault_status()
    with pytest.raises(ValueError):
        context.Context(device='cpu')


def test_context_on_a_second_device(S):
    _lib, batch, context, synthetic = S
    if torch.cuda.device_count() < 2:
        pytest.skip('needs two GPUs')
    torch.cuda.set_device(0)
    scenes = [synthetic.make_scene(CFG, 40 + e) for e in range(2)]
    with context.Context('cuda:1') as c:
        assert c.device == torch.device('cuda:1')
        with pytest.raises(ValueError):
            batch.StateBatch(scenes, device='cuda:0', context=c)
        b = batch.StateBatch(scenes, device='cuda:1', context=c)
        st = b.as_hwc(b.render()).cpu().numpy()
        assert torch.cuda.current_device() == 0
        for n, (e, x) in enumerate(b.agents):
            assert _same(st[n], O.agent_state(scenes[e], x)), n
        assert c.fault_status() == 0
    assert torch.cuda.current_device() == 0
