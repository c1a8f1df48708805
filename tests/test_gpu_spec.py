"""GPU: the compile-time instances of get_state_kernel (include/simaps_spec.h, csrc/simaps_spec.hip)
against the generic kernel of the same build.

A render() without debug buffers of a standard stack launches an instance (the query says which);
render(debug=alloc_debug()) is the generic kernel.  The two states must be torch.equal.  Cases: the
small room (early_tile / tail_cells, 1-cell column sweeps), the 92 x 92 room (the other tile /
code-map layout, 2-cell sweeps), the one-source stack with 12 render waves (S2), a subset render of
32 seeded stacks, the configurations no instance covers (the fallback), and a descriptor clamp,
which must post the same fault word and `where` through an instance as through the generic kernel.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FLAGSHIP = 'lifting_4-small_divider'


@pytest.fixture(scope='module')
def S():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a GPU (run with -m gpu on an MI355X)')
    from simaps import _lib, batch, context, synthetic
    _lib.lib.simaps_fault_status(1)
    yield _lib, batch, context, synthetic
    _lib.lib.simaps_fault_status(1)


def _both(S, b, want, slots=None):
    """(instance render, generic render, debug outputs) of batch b; the instance id must be `want`."""
    _lib = S[0]
    assert b.kernel_instance() == want
    assert b.kernel_instance(debug=True) == _lib.SPEC_GENERIC
    n = b.N if slots is None else len(slots)
    dbg = b.alloc_debug(n)
    spec = b.render(slots=slots)
    gen = b.render(debug=dbg, slots=slots)
    torch.cuda.synchronize()
    _lib.check_faults()
    assert spec.dtype == torch.float32 and tuple(spec.shape) == b.out_shape(n)
    return spec, gen, dbg


@pytest.mark.parametrize('name, want', [(FLAGSHIP, 1), ('pushing_4-large_empty', 1), ('rescue_4-small_empty', 2)])
def test_instance_equals_generic_one_env(S, name, want):
    _lib, batch, context, synthetic = S
    b = batch.StateBatch([synthetic.make_scene(name, 0)])
    assert b.N == 4 and bool(b.cfg.layout_chw)
    spec, gen, dbg = _both(S, b, want)
    assert torch.equal(spec, gen)
    assert not torch.isnan(spec).any() and float(spec.abs().max()) > 0
    nsrc = (dbg['sources'][:, :, 0] >= 0).sum(1).cpu().numpy()
    assert (nsrc == (2 if want == 1 else 1)).all()                      # S1: two sources, S2: one


def _near_walls(scene, seed):
    """Robots 2 and 3 of the scene moved anywhere in the room up to 2 cm from its edge (the recipe of
    tools/fuzz_states.py --perturb): next to a wall or on the divider the robot's pixel is outside the
    configuration space, so its shortest-path source is snapped to the closest free cell."""
    rs = np.random.RandomState(seed)
    rl, rw = scene['room_length'], scene['room_width']
    for r in scene['robots'][2:]:
        r['position'] = (float(rs.uniform(-rl / 2 + 0.02, rl / 2 - 0.02)),
                         float(rs.uniform(-rw / 2 + 0.02, rw / 2 - 0.02)), 0)
        r['waypoint_positions'] = [r['position']] + list(r['waypoint_positions'][1:])
    return scene


def test_instance_equals_generic_subset_of_32_stacks(S):
    """8 seeded envs of the flagship (32 stacks), two robots of each moved next to walls, a subset of
    19 map slots in shuffled order: stacks that converge in 3 and in 4 SSSP rounds, snapped sources."""
    _lib, batch, context, synthetic = S
    b = batch.StateBatch([_near_walls(synthetic.make_scene(FLAGSHIP, 100 + e), 100 + e) for e in range(8)])
    assert b.N == 32
    slots = [int(k) for k in np.random.RandomState(4).permutation(32)[:19]]
    spec, gen, dbg = _both(S, b, 1, slots=slots)
    assert torch.equal(spec, gen)
    full, gen_full, dbg_full = _both(S, b, 1)
    assert torch.equal(full, gen_full)
    assert torch.equal(full[torch.as_tensor(slots, device=full.device)], spec)
    st = dbg_full['status'].cpu().numpy()
    src = dbg_full['sources'].cpu().numpy()
    rounds, snapped = set((st >> 8).tolist()), int((src[:, :, :2] != src[:, :, 2:]).any(2).sum())
    print('rounds per stack:', sorted(rounds), 'snapped sources:', snapped)
    assert {3, 4} <= rounds and snapped > 0                              # what this case is there to cover
    assert ((st & 14) == 0).all()                                        # no round cap, timeout or clamp


@pytest.mark.parametrize('name', ['lifting_4-small_divider-history', 'lifting_4-small_divider-spatial'])
def test_other_configurations_take_the_generic_kernel(S, name):
    _lib, batch, context, synthetic = S
    b = batch.StateBatch([synthetic.make_scene(name, 0)])
    plain, gen, _ = _both(S, b, _lib.SPEC_GENERIC)
    assert torch.equal(plain, gen)


def test_hwc_layout_takes_the_generic_kernel(S):
    _lib, batch, context, synthetic = S
    scene = synthetic.make_scene(FLAGSHIP, 0)
    hwc = batch.StateBatch([scene], layout='hwc')
    chw = batch.StateBatch([scene])
    plain, gen, _ = _both(S, hwc, _lib.SPEC_GENERIC)
    assert torch.equal(plain, gen)
    assert torch.equal(chw.as_hwc(chw.render()), plain)                 # S1 (chw) against the generic HWC render


def test_descriptor_clamp_posts_the_same_fault_through_an_instance(S):
    """An agent's robot index past num_robots (the recipe of tests/test_gpu_ctx.py): the kernel clamps
    it, finishes normally and posts SIMAPS_FAULT_DESCRIPTOR with `where` = (get_state, the agent)."""
    _lib, batch, context, synthetic = S
    b = batch.StateBatch([synthetic.make_scene(FLAGSHIP, 7 + e) for e in range(2)])
    robots, envs, ag, paths = batch.pack_descriptors(b.scenes, b.agents)
    robots = np.concatenate([robots, np.repeat(robots[:1], 8)])
    paths = np.concatenate([paths, np.repeat(paths[:1], 40, 0)])
    ag['robot'][5] = 6                                                   # 8 agents, only agent 5 is bad
    R, E, A = (batch._to_dev(x, b.device) for x in (robots, envs, ag))
    P = torch.from_numpy(paths).to(b.device)
    status = torch.zeros(b.N, dtype=torch.int32, device=b.device)
    dbg = _lib.Debug(None, None, None, status.data_ptr(), None)
    assert _lib.lib.simaps_get_state_instance(b.cfg, 0) == _lib.SPEC_S1
    assert _lib.lib.simaps_get_state_instance(b.cfg, 1) == _lib.SPEC_GENERIC
    ctx = context.Context()
    try:
        got = []
        for d in (None, dbg):                                            # S1, then the generic kernel
            out = b.alloc_state()
            rc = _lib.call(ctx, 'get_state', b.cfg, b.N, _lib.ptr(A), _lib.ptr(E), _lib.ptr(R), _lib.ptr(P),
                           _lib.ptr(b.occupancy), _lib.ptr(b.overhead), _lib.ptr(out), 0, d, _lib.stream_handle())
            assert rc == 0
            torch.cuda.synchronize()
            k, u = ctypes.c_int(-2), ctypes.c_int(-2)
            bits = _lib.lib.simaps_ctx_fault_info(ctx.handle, 0, ctypes.byref(k), ctypes.byref(u))
            info = ctx.fault_info(clear=True)
            got.append((bits, k.value, u.value, info, out))
        (b1, k1, u1, i1, o1), (b2, k2, u2, i2, o2) = got
        assert (b1, k1, u1) == (b2, k2, u2) == (_lib.FAULT_DESCRIPTOR, 1, 5)     # SIMAPS_K_GET_STATE, agent 5
        assert i1 == i2 == (_lib.FAULT_DESCRIPTOR, 'get_state', 5)
        assert torch.equal(o1, o2)
        assert int(status[5]) & 8 and not (status.cpu().numpy()[[0, 1, 2, 3, 4, 6, 7]] & 8).any()
    finally:
        torch.cuda.synchronize()
        ctx.fault_status(clear=True)
        ctx.close()
