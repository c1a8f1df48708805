"""GPU: get_state AT its descriptor limits -- SIMAPS_MAX_ROBOTS = 8 robots per env, SIMAPS_MAX_PATH =
16 points per path, all 120 segment slots -- against the oracle (pinned at these sizes by the
scene_dense_* goldens, tests/test_oracle_golden.py) with the rule of tests/test_gpu_parity.py: bit for
bit, the nonspatial intention channels within 1e-7.

The scenes are tests/dense_scenes.py's (tests/test_dense_scenes.py shows on the CPU that the upper
segment slots 64..119 are visible in the stacks).  What runs only here: raster_lines' second scan half
(slots 64..119), the params-phase segment lanes 384..439, seg_table on lanes 4..7, the channel order
beyond 3 other robots and with equal distances, the robot stamps of groups 3 and 4 -- in the generic
kernel, the S1 / S2 instances and their room-class twins, the 16-bit and store launches, the mixed
launch and simaps_global_maps.

Every test renders 2 envs (at most 16 stacks); the oracle's stacks are computed once per (case,
rounding) and shared."""
import functools

import numpy as np
import pytest
import torch

import dense_scenes as D
import oracle as O
from test_gpu_parity import _bitwise, _check_state
from test_spec_store_abi import FAMILIES

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ['f32', 'bf16', 'f16']
LAUNCH_CASES = ['s1_small_8', 's2_small_8', 'all_8x4groups', 'ragged_8']


@pytest.fixture(scope='module')
def S():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a GPU (run with -m gpu on an MI355X)')
    from simaps import _lib, batch, synthetic
    _lib.lib.simaps_fault_status(1)
    yield _lib, batch, synthetic
    _lib.lib.simaps_fault_status(1)


@functools.lru_cache(maxsize=None)
def _ref(name, rounding, e, a):
    st = O.agent_state(D.scenes(name, rounding)[e], a)
    st.setflags(write=False)
    return st


def ints(t):
    """The integer view of a float32 / bf16 / fp16 tensor, on the host."""
    t = t.detach().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu().numpy()


def _expect(S, b, name, dtype=None, into=False):
    """The queries say the case's instance and room class (and the generic kernel with a debug output)."""
    _lib = S[0]
    c = D.CASES[name]
    assert (D.GENERIC, D.S1, D.S2, D.ROOM_NONE, D.ROOM_SMALL) == (_lib.SPEC_GENERIC, _lib.SPEC_S1, _lib.SPEC_S2,
                                                                  _lib.ROOM_NONE, _lib.ROOM_SMALL)
    on = (dtype in (None, torch.float32) and not into) or FAMILIES['into' if into else 'plain16']
    want = (c.instance, c.room) if on else (D.GENERIC, D.ROOM_NONE)
    assert (b.kernel_instance(dtype=dtype, into=into), b.room_class(dtype=dtype, into=into)) == want
    assert (b.kernel_instance(debug=True, dtype=dtype, into=into),
            b.room_class(debug=True, dtype=dtype, into=into)) == (D.GENERIC, D.ROOM_NONE)


def _clean_status(status):
    st = status.cpu().numpy()
    assert (st & 0xff == 0).all(), 'status bits %s' % sorted(set((st & 0xff).tolist()))  # bit 3: descriptor clamped


@pytest.mark.parametrize('rounding', ['fma', 'plain'])
@pytest.mark.parametrize('name', D.CASE_IDS)
def test_dense_case_matches_the_oracle(S, name, rounding):
    """One render with a status buffer (the generic kernel), one without (the case's instance): no
    status bit -- a 16-point path is at the limit, not past it -- the two are equal bit for bit, and
    every stack is the oracle's."""
    _lib, batch, synthetic = S
    scenes = D.scenes(name, rounding)
    b = batch.StateBatch(scenes)
    assert b.N == sum(len(s['robots']) for s in scenes) <= 16 and bool(b.cfg.layout_chw)
    assert b.cfg.rotate_rounding == _lib.ROT_IDS[rounding]
    _expect(S, b, name)
    status = torch.full((b.N,), -1, dtype=torch.int32, device=b.device)
    gen = b.render(debug={'status': status})
    inst = b.render()
    torch.cuda.synchronize()
    _clean_status(status)
    got = b.as_hwc(inst).cpu().numpy()
    flags = scenes[0]['flags']
    for n, (e, a) in enumerate(b.agents):
        _check_state(got[n], _ref(name, rounding, e, a), flags, len(scenes[e]['robots']))
    assert np.array_equal(ints(gen), ints(inst))
    _lib.check_faults()


_BATCH = {}


def _batch(S, name):
    """(scenes, StateBatch, its float32 render) of a case in the fused rounding, made once."""
    if name not in _BATCH:
        _lib, batch, synthetic = S
        scenes = D.scenes(name)
        b = batch.StateBatch(scenes)
        f32 = b.render()
        torch.cuda.synchronize()
        _BATCH[name] = (scenes, b, f32)
    return _BATCH[name]


@pytest.mark.parametrize('dtype', DTYPES[1:], ids=IDS[1:])
@pytest.mark.parametrize('name', LAUNCH_CASES)
def test_dense_16_bit_render_is_the_cast_float32_render(S, name, dtype):
    _lib = S[0]
    scenes, b, f32 = _batch(S, name)
    _expect(S, b, name, dtype=dtype)
    status = torch.full((b.N,), -1, dtype=torch.int32, device=b.device)
    inst = b.render(dtype=dtype)
    gen = b.render(dtype=dtype, debug={'status': status})
    torch.cuda.synchronize()
    _clean_status(status)
    assert inst.dtype == dtype and tuple(inst.shape) == b.out_shape(b.N)
    want = ints(f32.cpu().to(dtype))
    assert np.array_equal(ints(inst), want)
    assert np.array_equal(ints(gen), want)
    _lib.check_faults()


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('name', LAUNCH_CASES)
def test_dense_render_into_a_store(S, name, dtype):
    """dest: a permutation of the store's rows with two agents skipped (-1).  The rows written are
    render()'s stacks in the store's dtype, every other row keeps its sentinel."""
    _lib = S[0]
    scenes, b, f32 = _batch(S, name)
    _expect(S, b, name, dtype=dtype, into=True)
    capacity = b.N + 3
    dest = np.random.RandomState(b.N + len(name)).permutation(capacity)[:b.N].astype(np.int64)
    dest[[3, b.N - 1]] = -1                                              # agent (0, 3) and the last agent of env 1
    it, fill = (torch.int32, 0x5A5A5A5A) if dtype == torch.float32 else (torch.int16, 0x5A5A)
    stores = []
    for debug in (None, {'status': torch.full((b.N,), -1, dtype=torch.int32, device=b.device)}):
        buf = torch.full((capacity * 96 * 96 * b.C,), fill, dtype=it, device=b.device)
        store = buf.view(dtype).view(b.out_shape(capacity))
        assert b.render_into(store, torch.from_numpy(dest).to(b.device), debug=debug) is store
        stores.append(ints(store))
    torch.cuda.synchronize()
    want = ints(f32.cpu().to(dtype))
    for got in stores:
        for n, r in enumerate(dest):
            if r >= 0:
                assert np.array_equal(got[r], want[n]), (n, r)
        for r in sorted(set(range(capacity)) - set(dest.tolist())):
            assert (got[r] == fill).all(), 'row %d was written' % r
    _lib.check_faults()


def test_dense_mixed_launch_equals_per_configuration_renders(S):
    """all_8x4groups, spatial_5, s1_small_8 and the stock lifting_4-small_divider, env by env
    interleaved, in one launch: float32 and bfloat16, bit for bit one StateBatch render each."""
    _lib, batch, synthetic = S
    per = [D.scenes('all_8x4groups'), D.scenes('spatial_5'), D.scenes('s1_small_8'),
           [synthetic.make_scene('lifting_4-small_divider', 520 + e) for e in range(2)]]
    scenes = [p[e] for e in range(2) for p in per]
    mb = batch.MixedStateBatch(scenes)
    assert len(mb.plan['cfgs']) == 4 and mb.N == 2 * (8 + 5 + 8 + 4)
    groups = {}
    for e, s in enumerate(scenes):
        groups.setdefault(batch.config_key(s), []).append(e)
    assert len(groups) == 4
    for dtype in (torch.float32, torch.bfloat16):
        views = [ints(v) for v in mb.states(mb.render(dtype=dtype))]
        want = {}
        for envs in groups.values():
            b = batch.StateBatch([scenes[e] for e in envs])
            st = ints(b.render(dtype=dtype))
            for n, (i, a) in enumerate(b.agents):
                want[(envs[i], a)] = st[n]
        for n, (e, a) in enumerate(mb.agents):
            assert np.array_equal(views[n], want[(e, a)]), (dtype, n, e, a)
    _lib.check_faults()


@pytest.mark.parametrize('name', ['all_8x4groups', 'binary_t2_8'])
def test_dense_global_maps(S, name):
    """simaps_global_maps (seg_table on lanes 4..7, the stamps of groups 3 and 4) for every agent:
    the oracle's whole-grid overhead, robot, history and intention maps, bit for bit."""
    _lib, batch, synthetic = S
    scenes = D.scenes(name)
    b = batch.StateBatch(scenes)
    g = {k: v.cpu().numpy() for k, v in b.global_maps().items()}
    _lib.check_faults()
    f = scenes[0]['flags']
    assert set(g) == {'overhead', 'robot', 'intention'} | ({'history'} if f['use_history_map'] else set())
    for n, (e, a) in enumerate(b.agents):
        ao = O.AgentOracle(scenes[e], a)
        want = {'overhead': ao.global_overhead_map(), 'robot': ao.global_robot_map(seg=False),
                'intention': ao.global_intention_map(f['intention_map_encoding'])}
        if f['use_history_map']:
            want['history'] = ao.global_intention_map('history')
        for k, w in want.items():
            assert _bitwise(g[k][n], w.astype(np.float32)), (name, e, a, k)
    if name == 'all_8x4groups':
        assert {7 / 8, 1.0} <= set(np.unique(g['overhead']).tolist())


def test_dense_awaiting_subset(S):
    """s1_small_8, only agents (0, 7), (1, 4), (0, 5): as slots of the whole batch and as a batch of
    those three alone (agent 7 is the last robot record, sh.me = 7)."""
    _lib, batch, synthetic = S
    scenes, b, f32 = _batch(S, 's1_small_8')
    agents = [(0, 7), (1, 4), (0, 5)]
    slots = [b.agents.index(x) for x in agents]
    sub = b.as_hwc(b.render(slots=slots)).cpu().numpy()
    own = batch.StateBatch(scenes, agents=agents)
    _expect(S, own, 's1_small_8')
    alone = own.as_hwc(own.render()).cpu().numpy()
    torch.cuda.synchronize()
    for n, (e, a) in enumerate(agents):
        assert _bitwise(sub[n], _ref('s1_small_8', None, e, a)), (e, a)
        assert _bitwise(alone[n], _ref('s1_small_8', None, e, a)), (e, a)
    _lib.check_faults()


@pytest.mark.parametrize('name', ['s1_small_8', 'all_8x4groups'])
def test_dense_array_descriptors_render_the_same(S, name):
    """The per-step array path (simaps_pack_robots: fixed 16-point strides, here every one full; 30
    waypoints per robot for all_8x4groups) renders what the scene descriptors rendered."""
    _lib, batch, synthetic = S
    scenes, _, f32 = _batch(S, name)
    b = batch.StateBatch(scenes)
    b.set_descriptor_arrays(**batch.descriptor_arrays(scenes))
    assert np.array_equal(ints(b.render()), ints(f32))
    _lib.check_faults()
