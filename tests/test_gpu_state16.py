"""GPU: the state stack rendered directly as bf16 / fp16 (include/simaps_state16.h,
StateBatch.render(dtype=...)) is bit for bit the float32 render cast by torch -- every comparison here
is on the int16 views and exact -- and everything beside the stack (debug outputs, receptacle cache,
faults) is the float32 call's.

The scenes are the golden one-env scenes of tests/goldens.py, at most 4 agents per launch.
"""
import os

import numpy as np
import pytest
import torch

import goldens as G
import oracle as O

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
LAYOUTS = ['chw', 'hwc']
CFG = 'lifting_4-small_divider'


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
    """(scene, golden agents) of env 0 of tests/golden/scene_<cfg>.npz (a fresh shallow copy of the scene)."""
    if not _GOLD:
        for _, e, a, scene, _, z in G.scene_cases():
            if e == 0:
                stem = os.path.splitext(os.path.basename(z.zip.filename))[0][len('scene_'):]
                _GOLD.setdefault(stem, (scene, []))[1].append(a)
    scene, agents = _GOLD[cfg]
    return dict(scene), [(0, a) for a in agents]


def first_robots(scene, agents, n):
    """The scene with its first n robots only (another robot count: another C with intention channels)."""
    s = dict(scene, robots=scene['robots'][:n], occupancy=scene['occupancy'][:n], overhead=scene['overhead'][:n])
    return s, [(e, a) for e, a in agents if a < n]


def all_agents(scene, agents):
    """Every robot of the scene as an agent: the goldens carry the maps of some agents only, the others
    get a copy of the first golden agent's (each robot maps the same room)."""
    have = [a for _, a in agents]
    occ, ovh = scene['occupancy'].copy(), scene['overhead'].copy()
    for a in range(len(scene['robots'])):
        if a not in have:
            occ[a], ovh[a] = occ[have[0]], ovh[have[0]]
    return dict(scene, occupancy=occ, overhead=ovh), [(0, a) for a in range(len(scene['robots']))]


def i16(t):
    """The int16 view of a 16-bit tensor, on the host."""
    assert t.dtype in DTYPES
    return t.contiguous().view(torch.int16).cpu().numpy()


def cast16(f32, dtype):
    """The oracle: torch's CPU cast of the float32 render."""
    return i16(f32.detach().cpu().to(dtype))


def _parity_cases():
    all_off = {k: False for k in ('use_robot_map', 'use_distance_to_receptacle_map',
                                  'use_shortest_path_to_receptacle_map', 'use_shortest_path_map', 'use_intention_map',
                                  'use_history_map', 'use_intention_channels')}
    return {
        'all_off': lambda: (lambda s, a: (dict(s, flags=dict(s['flags'], **all_off)), a))(*golden(CFG)),
        'all': lambda: golden('lifting_2_pushing_2-large_empty-all'),
        'history_intention': lambda: (lambda s, a: (dict(s, flags=dict(s['flags'], use_history_map=True)), a))(*golden(CFG)),
        'spatial_4': lambda: golden('lifting_4-small_divider-spatial'),
        'spatial_3': lambda: first_robots(*golden('lifting_4-small_divider-spatial'), 3),
        'nonspatial_4': lambda: golden('lifting_4-large_empty-nonspatial'),
        'nonspatial_3': lambda: first_robots(*golden('lifting_4-large_empty-nonspatial'), 3),
    }


PARITY = _parity_cases()
WANT_C = {'all_off': 1, 'all': 10, 'history_intention': 6, 'spatial_4': 7, 'spatial_3': 6, 'nonspatial_4': 10,
          'nonspatial_3': 8}


@pytest.mark.parametrize('name', sorted(PARITY))
def test_parity_with_the_cast_of_the_float32_render(S, name):
    """render(dtype) == render().to(dtype), both layouts, over the flag combinations; the odd channel
    counts (all_off 1, spatial_4 7) put an HWC pixel's first element off a 4-byte boundary."""
    _lib, batch, context, vector_env = S
    scene, agents = PARITY[name]()
    assert 1 <= len(agents) <= 4
    for layout in LAYOUTS:
        b = batch.StateBatch([scene], agents=agents, layout=layout)
        assert b.C == WANT_C[name]
        f32 = b.render()
        torch.cuda.synchronize()
        assert f32.dtype == torch.float32 and float(f32.abs().max()) > 0
        for dtype in DTYPES:
            got = b.render(dtype=dtype)
            assert got.dtype == dtype and tuple(got.shape) == tuple(f32.shape)
            assert np.array_equal(i16(got), cast16(f32, dtype)), (name, layout, dtype)
            out = b.alloc_state(dtype=dtype)
            assert b.render(out=out) is out
            assert np.array_equal(i16(out), cast16(f32, dtype))
    with pytest.raises(ValueError):
        b.render(dtype=torch.float64)
    with pytest.raises(ValueError):
        b.render(out=torch.empty(b.out_shape(), dtype=torch.int16, device=b.device))
    with pytest.raises(ValueError):
        b.render(out=b.alloc_state(dtype=torch.float16), dtype=torch.bfloat16)
    torch.cuda.synchronize()
    assert _lib.lib.simaps_fault_status(0) == 0


def _f32(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


# float32 bit patterns, one per rounding class (bf16 keeps the top 16 bits, ties at 0x8000 below;
# fp16 keeps 10 mantissa bits, ties at 0x1000 in the 13 dropped)
CRAFTED = np.concatenate([
    _f32([0x3F808000, 0x3F807FFF, 0x3F808001]),          # bf16 tie, even kept mantissa (stays), and one ulp to either side
    _f32([0x3F818000, 0x3F817FFF, 0x3F818001]),          # bf16 tie, odd kept mantissa (rounds up), and either side
    _f32([0x3F801000, 0x3F800FFF, 0x3F801001]),          # fp16 tie, even
    _f32([0x3F803000, 0x3F802FFF, 0x3F803001]),          # fp16 tie, odd
    np.array([1e-6, 5.9e-8, 2.9e-8, -1e-6], np.float32),  # fp16 subnormals, the least one, below half of it (-> 0)
    _f32([0x33000000, 0x33000001, 0x33C00000]),          # 2^-25: tie between 0 and the least subnormal; just above; 3 * 2^-25: tie up to even
    _f32([0x387FC000, 0x387FE000]),                      # largest fp16 subnormal; the tie up to the least normal
    np.array([65504.0, 65520.0, 7e4, -65520.0], np.float32),  # fp16 max; the tie that overflows; beyond; its negative
    _f32([0x477FEFFF]),                                  # 65519.996: the last float32 that stays finite in fp16
    _f32([0x00000000, 0x80000000]),                      # +-0.0
    _f32([0x00400000, 0x00018000, 0x00000001, 0x80400000]),  # float32 subnormals (bf16 keeps / rounds them, fp16: +-0)
    _f32([0x7F800000, 0xFF800000]),                      # +-inf
    _f32([0x7F7FFFFF]),                                  # float32 max: overflows in both formats
])


def oracle_channel_0(scene, agent):
    """The CPU oracle's channel 0 (AgentOracle.get_state: _local_map(global_overhead_map())), from the
    oracle's own steps without global_overhead_map's `max() <= 1` assertion, which the reference makes
    of its segmentation codes and the crafted patterns (65504, inf) are outside of."""
    ao = O.AgentOracle(scene, agent)
    g = ao.overhead_wo.copy()
    seg = ao.global_robot_map(seg=True)
    g[seg > 0] = seg[seg > 0]
    return np.ascontiguousarray(ao._local_map(g))


def test_rounding_classes_through_channel_0(S):
    """The overhead map passes through the rotated gather verbatim, so crafted float32 bit patterns
    tiled over one slot's map reach the store: ties to even, fp16 subnormals and overflow, signed
    zeros, float32 subnormals, infinities."""
    _lib, batch, context, vector_env = S
    assert len(CRAFTED) == 35 and not np.isnan(CRAFTED).any()
    assert {2.0 ** -25, 3 * 2.0 ** -25, 1023 * 2.0 ** -24, 65520.0, 65504.0} <= set(float(x) for x in CRAFTED)
    want_bits = np.unique(CRAFTED.view(np.uint32))
    assert len(want_bits) == len(CRAFTED)
    scene, agents = golden(CFG)
    a0 = agents[0][1]
    H, W = scene['H'], scene['W']
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    ovh = scene['overhead'].copy()
    ovh[a0] = CRAFTED[(ii * 7 + jj) % len(CRAFTED)]      # every pattern in every 35 consecutive pixels of a row
    scene['overhead'] = ovh
    # on the CPU first: the oracle's channel 0 of this scene already holds every pattern
    ref0 = oracle_channel_0(scene, a0)
    assert np.isin(want_bits, ref0.view(np.uint32)).all()
    # torch's CPU cast is the IEEE round-to-nearest-even one (NumPy's for fp16; bf16 restated in integers)
    c = torch.from_numpy(CRAFTED.copy())
    with np.errstate(over='ignore'):                         # (the overflow to inf is one of the classes)
        np16 = CRAFTED.astype(np.float16)
    assert np.array_equal(c.to(torch.float16).view(torch.int16).numpy(), np16.view(np.int16))
    u = CRAFTED.view(np.uint32).astype(np.uint64)
    rne = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    assert np.array_equal(c.to(torch.bfloat16).view(torch.int16).numpy(), rne.view(np.int16))
    for layout in LAYOUTS:
        b = batch.StateBatch([scene], agents=[(0, a0)], layout=layout)
        f32 = b.render()
        torch.cuda.synchronize()
        ch0 = np.ascontiguousarray(b.as_hwc(f32)[0, :, :, 0].cpu().numpy())
        assert np.isin(want_bits, ch0.view(np.uint32)).all()     # never an empty comparison
        assert np.array_equal(ch0.view(np.uint32), ref0.view(np.uint32))
        for dtype in DTYPES:
            got = b.render(dtype=dtype)
            assert np.array_equal(i16(got), cast16(f32, dtype)), (layout, dtype)
            g0 = b.as_hwc(got)[0, :, :, 0].float().cpu().numpy()
            assert np.isinf(g0).any() and (g0 == 0).any()


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'f16'])
@pytest.mark.parametrize('layout', LAYOUTS)
def test_no_stray_bytes(S, layout, dtype):
    """N = 1, N = 3 and a permuted `slots` subset into the middle of a larger sentinel-filled buffer: the
    bytes before and after the N stacks stay, and each stack is its own slot's cast."""
    _lib, batch, context, vector_env = S
    scene, agents = all_agents(*golden('lifting_4-small_divider-spatial'))   # C = 7: an odd pixel length in HWC
    b = batch.StateBatch([scene], agents=agents, layout=layout)
    assert b.N == 4 and b.C == 7
    f32 = b.render()
    torch.cuda.synchronize()
    want = cast16(f32, dtype)
    stack = 96 * 96 * b.C
    for slots in ([2], [3, 0, 2], [1, 3]):
        n = len(slots)
        buf = torch.full(((n + 2) * stack,), 0x5A5A, dtype=torch.int16, device=b.device)
        out = buf[stack:(n + 1) * stack].view(dtype).view(b.out_shape(n))
        assert out.data_ptr() % 16 == 0
        b.render(out=out, slots=slots)
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        assert (host[:stack] == 0x5A5A).all() and (host[(n + 1) * stack:] == 0x5A5A).all(), slots
        for k, s in enumerate(slots):
            assert np.array_equal(host[(k + 1) * stack:(k + 2) * stack], want[s].reshape(-1)), (slots, k)
    # N = 1 as a whole batch of its own
    b1 = batch.StateBatch([scene], agents=agents[1:2], layout=layout)
    buf = torch.full((3 * stack,), 0x5A5A, dtype=torch.int16, device=b.device)
    b1.render(out=buf[stack:2 * stack].view(dtype).view(b1.out_shape()))
    host = buf.cpu().numpy()
    assert (host[:stack] == 0x5A5A).all() and (host[2 * stack:] == 0x5A5A).all()
    assert np.array_equal(host[stack:2 * stack], want[1].reshape(-1))


def _bytes(t):
    return t.contiguous().view(torch.uint8).cpu().numpy()


def test_side_outputs_are_the_float32_calls(S):
    """Debug cspace / sources / dist / status and the receptacle cache records: bitwise those of the
    float32 render; receptacle_distances answers the same after a bf16 render."""
    _lib, batch, context, vector_env = S
    scene, agents = golden(CFG)
    rs = np.random.RandomState(5)
    tgt = rs.uniform(-0.4, 0.4, size=(len(agents), 3, 2))
    res = {}
    for dtype in [torch.float32] + DTYPES:
        b = batch.StateBatch([scene], agents=agents)
        rec = b.enable_receptacle_cache()
        rec.zero_()
        dbg = {k: torch.zeros_like(v) for k, v in b.alloc_debug().items()}
        b.render(debug=dbg, dtype=dtype)
        torch.cuda.synchronize()
        assert (b._rec_ver == b._map_ver).all()                   # the records count as current: a lookup next
        d = b.receptacle_distances(tgt)
        res[dtype] = dict({k: _bytes(v) for k, v in dbg.items()}, rec=_bytes(rec), lookup=_bytes(d))
        if dtype == torch.float32:
            res['full'] = _bytes(b.receptacle_distances(tgt, cache=False))
    f = res[torch.float32]
    assert f['rec'].any() and f['cspace'].any() and f['dist'].any() and (f['status'].view(np.int32) & 0xff == 0).all()
    assert np.array_equal(f['lookup'], res['full'])
    for dtype in DTYPES:
        for k in ('cspace', 'sources', 'dist', 'status', 'rec', 'lookup'):
            assert np.array_equal(res[dtype][k], f[k]), (dtype, k)


def _get_state_as(S, ctx, b, R, E, A, P, out, dtype_id):
    _lib = S[0]
    return _lib.call(ctx, 'get_state_as', b.cfg, b.N, _lib.ptr(A), _lib.ptr(E), _lib.ptr(R), _lib.ptr(P),
                     _lib.ptr(b.occupancy), _lib.ptr(b.overhead), _lib.ptr(out), dtype_id, 0, None,
                     _lib.stream_handle())


def test_f32_dispatch_is_simaps_get_state(S):
    _lib, batch, context, vector_env = S
    scene, agents = golden(CFG)
    b = batch.StateBatch([scene], agents=agents)
    want = b.render()
    good = (b.robots_d, b.envs_d, b.agents_d, b.paths_d)
    ctx = context.Context()
    try:
        for c in (None, ctx):
            out = torch.full_like(want, float('nan'))
            assert _get_state_as(S, c, b, *good, out, _lib.STATE_F32) == 0
            torch.cuda.synchronize()
            assert np.array_equal(_bytes(out), _bytes(want))
        assert ctx.fault_info() == (0, None, None)
    finally:
        ctx.close()


def test_descriptor_fault_goes_to_the_calling_context_only(S):
    """A robot index >= num_robots (the clamped-descriptor case of tests/test_gpu_ctx.py: the kernel
    clamps, finishes normally and reports) through a Context: SIMAPS_FAULT_DESCRIPTOR with kernel id
    SIMAPS_K_GET_STATE and that agent's index, in that context only; the other stacks are their casts."""
    _lib, batch, context, vector_env = S
    scene, agents = all_agents(*golden(CFG))
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
    a, other = context.Context(), context.Context()
    try:
        for dtype in DTYPES:
            out = b.alloc_state(dtype=dtype)
            assert _get_state_as(S, a, b, R, E, A, P, out, _lib.state_dtype_id(dtype)) == 0
            torch.cuda.synchronize()
            assert a.fault_info() == (_lib.FAULT_DESCRIPTOR, 'get_state', bad)
            assert _lib.K_NAMES[1] == 'get_state'
            assert other.fault_info() == (0, None, None) and _lib.lib.simaps_fault_status(0) == 0
            assert a.fault_info(clear=True)[0] == _lib.FAULT_DESCRIPTOR
            got, ref = i16(out), cast16(want, dtype)
            for n in range(b.N):
                if n != bad:
                    assert np.array_equal(got[n], ref[n]), (dtype, n)
    finally:
        torch.cuda.synchronize()
        for c in (a, other):
            c.fault_status(clear=True)
            c.close()


def _moved(scene):
    """The scene one step later: every robot turned and shifted a little (same maps)."""
    robots = [dict(r, heading=r['heading'] + 0.4, position=(r['position'][0] + 0.03, r['position'][1] - 0.02) +
                   tuple(r['position'][2:])) for r in scene['robots']]
    return dict(scene, robots=robots)


def test_graph_capture_replays_after_a_descriptor_update(S):
    _lib, batch, context, vector_env = S
    scene, agents = golden(CFG)
    b = batch.StateBatch([scene], agents=agents)
    b.set_descriptor_arrays(**batch.descriptor_arrays([scene]))       # fixed-size device descriptors
    first = b.render(dtype=torch.bfloat16).clone()
    out = b.alloc_state(dtype=torch.bfloat16)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        b.render(out=out)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(i16(out), i16(first))
    # the next step's descriptor, written in place into the buffers the captured launch reads
    rob, pth = b.robots_d, b.paths_d
    b.set_descriptor_arrays(**batch.descriptor_arrays([_moved(scene)]))
    assert rob.shape == b.robots_d.shape and pth.shape == b.paths_d.shape
    rob.copy_(b.robots_d)
    pth.copy_(b.paths_d)
    eager = b.render(dtype=torch.bfloat16)
    torch.cuda.synchronize()
    assert not np.array_equal(i16(eager), i16(first))
    for _ in range(2):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(i16(out), i16(eager))
    assert _lib.lib.simaps_fault_status(0) == 0


def test_vector_env_dropin_float16_ring(S):
    """VectorEnvObservations(dtype=torch.float16, reuse_outputs=2): two steps return each step's own
    states (two ring slots), as device tensors and as np.float16 arrays; bf16 has no NumPy form."""
    _lib, batch, context, vector_env = S
    scene, _ = golden(CFG)
    steps = [scene, _moved(scene)]
    ref = vector_env.VectorEnvObservations([scene])
    want = []
    for s in steps:
        ref.update(scenes=[s])
        want.append([[st.cpu().to(torch.float16).view(torch.int16).numpy() for st in grp] for grp in ref.get_state()[0]])
    assert not all(np.array_equal(x, y) for gx, gy in zip(*want) for x, y in zip(gx, gy))
    for numpy in (False, True):
        v = vector_env.VectorEnvObservations([scene], dtype=torch.float16, reuse_outputs=2)
        got = []
        for s in steps:
            v.update(scenes=[s])
            got.append(v.get_state(numpy=numpy)[0])
        torch.cuda.synchronize()
        for k in range(2):                                            # step 0's states are still step 0's
            for grp, wgrp in zip(got[k], want[k]):
                for st, w in zip(grp, wgrp):
                    if numpy:
                        assert isinstance(st, np.ndarray) and st.dtype == np.float16 and st.shape == w.shape
                        assert np.array_equal(st.view(np.int16), w)
                    else:
                        assert st.dtype == torch.float16 and tuple(st.shape) == w.shape
                        assert np.array_equal(i16(st), w)
    # without the ring, and a subset of awaiting robots
    v = vector_env.VectorEnvObservations([steps[1]], dtype=torch.float16)
    aw = [[a == 1 for a in range(len(scene['robots']))]]
    sub = v.get_state(awaiting=aw, numpy=True)[0]
    flat_sub = [st for grp in sub for st in grp]
    flat_want = [w for grp in want[1] for w in grp]
    order = [a for grp in vector_env.robot_groups(scene) for a in grp]
    for st, w, a in zip(flat_sub, flat_want, order):
        assert (st is not None) == (a == 1)
        if st is not None:
            assert st.dtype == np.float16 and np.array_equal(st.view(np.int16), w)
    vb = vector_env.VectorEnvObservations([scene], dtype=torch.bfloat16, reuse_outputs=2)
    assert vb.get_state()[0][0][0].dtype == torch.bfloat16
    with pytest.raises(ValueError, match='bfloat16'):
        vb.get_state(numpy=True)
    with pytest.raises(ValueError):
        vector_env.VectorEnvObservations([scene], dtype=torch.float64)
