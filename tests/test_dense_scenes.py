"""CPU: the descriptor-limit scenes of tests/dense_scenes.py are what tests/test_gpu_dense.py needs
them to be -- conditions on the inputs and on the oracle, so that the GPU tests are not vacuous:

* the full cases reach SIMAPS_MAX_ROBOTS x (SIMAPS_MAX_PATH - 1) segment slots and the packers
  (batch.pack_descriptors, the native simaps_pack_robots) accept them;
* what the upper slots (64..119: robots 5, 6, 7, and robot 4's last ones) draw is visible in the
  agent's stack, so a kernel that lost them would differ from the oracle;
* ties_8 holds exact distance ties; all_8x4groups shows the segmentation values of groups 3 and 4.

The thresholds are the issue's (50 pixels for robots 5..7 together, 10 for the last robot alone); the
seeds of dense_scenes.CASES were chosen to meet them."""
import functools

import numpy as np
import pytest

import dense_scenes as D
import oracle as O
from simaps import _lib, batch, synthetic

# cases whose passes fill segment slots from paths (circle draws targets only; ties_8 has no path map)
SLOT_CASES = [n for n in D.CASE_IDS if D.path_passes(D.CASES[n].flags) and
              D.CASES[n].flags.get('intention_map_encoding') != 'circle']


@functools.lru_cache(maxsize=None)
def _state(name, e, agent, idle=()):
    s = D.scenes(name)[e]
    st = O.agent_state(D.with_idle(s, set(idle)) if idle else s, agent)
    st.setflags(write=False)
    return st


def test_case_table():
    assert set(D.GOLDEN_CASES) <= set(D.CASE_IDS) and set(D.FULL_CASES) <= set(D.CASE_IDS)
    want_robots = {'spatial_5': 5, 'spatial_7': 7}
    for name, c in D.CASES.items():
        sc = D.scenes(name)
        assert len(sc) == D.ENVS == 2
        for s in sc:
            assert len(s['robots']) == want_robots.get(name, D.MAX_ROBOTS) <= _lib.MAX_ROBOTS
            assert s['config'] == D.config_name(name) and s['env_name'] == c.env_name
            assert all(s['flags'][k] == v for k, v in c.flags.items())
        assert batch.config_key(sc[0]) == batch.config_key(sc[1])
    assert (D.MAX_ROBOTS, D.MAX_PATH) == (_lib.MAX_ROBOTS, _lib.MAX_PATH)
    assert [r['group_index'] for r in D.scenes('all_8x4groups')[0]['robots']] == [0, 0, 1, 1, 2, 2, 3, 3]
    assert D.scenes('all_8x4groups')[0]['flags']['use_distance_to_receptacle_map']
    s = D.scenes('all_8x4groups')[0]
    assert synthetic.num_channels(s['flags'], len(s['robots'])) == 21
    assert D.scenes('s2_small_8')[0]['receptacle_position'] is None


@pytest.mark.parametrize('name', D.FULL_CASES)
def test_limits_reached(name):
    """Every robot other than the agent is moving and brings a path of exactly SIMAPS_MAX_PATH points
    to every raster pass: 15 slots each, up to slot 119."""
    for s in D.scenes(name):
        nr = len(s['robots'])
        assert nr == D.MAX_ROBOTS and not any(r['idle'] for r in s['robots'])
        passes = D.path_passes(s['flags'])
        assert passes
        for enc in passes:
            for r in s['robots']:
                assert D.pass_points(r, enc) == D.MAX_PATH
            for agent in (0, nr - 1):
                slots = D.used_slots(s, agent, enc)
                assert len(slots) == D.SEG_PER_ROBOT * (nr - 1)
                assert sum(q >= 64 for q in slots) == (56 if agent == 0 else 41)
            assert max(D.used_slots(s, 0, enc)) == D.MAX_ROBOTS * D.SEG_PER_ROBOT - 1


def test_slot_patterns_of_the_sparse_cases():
    """spatial_5: robot 4's slots straddle lane 64; line_8: one slot per robot, 15 apart; ragged_8:
    full and empty ranges interleaved, two robots idle in env 1."""
    for s in D.scenes('spatial_5'):
        assert [q for q in D.used_slots(s, 0, 'ramp') if q >= 60] == list(range(60, 75))
    for s in D.scenes('spatial_7'):
        assert len(D.used_slots(s, 0, 'ramp')) == 90 and max(D.used_slots(s, 0, 'ramp')) == 104
    for s in D.scenes('line_8'):
        assert D.used_slots(s, 0, 'line') == [15 * k for k in range(1, 8)]
    want = [16, 2, 16, 3, 2, 16, 9, 16]
    for e, s in enumerate(D.scenes('ragged_8')):
        assert [D.pass_points(r, 'ramp') for r in s['robots']] == want
        assert [k for k, r in enumerate(s['robots']) if r['idle']] == ([] if e == 0 else [2, 5])
        live = [k for k in range(1, 8) if not s['robots'][k]['idle']]
        assert len(D.used_slots(s, 0, 'ramp')) == sum(want[k] - 1 for k in live)


@pytest.mark.parametrize('name', D.CASE_IDS)
def test_packers_accept_the_cases(name):
    """pack_descriptors raises no ValueError and simaps_pack_robots returns 0 (not SIMAPS_EUNSUPPORTED);
    the two agree on the path lengths, which are at most -- and in the full cases exactly -- 16."""
    scenes = D.scenes(name)
    agents = [(e, a) for e, s in enumerate(scenes) for a in range(len(s['robots']))]
    rob, envs, ag, paths = batch.pack_descriptors(scenes, agents)
    assert envs['num_robots'].max() <= _lib.MAX_ROBOTS
    d = batch.descriptor_arrays(scenes)
    R, P = len(rob), _lib.MAX_PATH
    tg = np.array([(_lib.TYPE_IDS[r['type']], r['group_index']) for s in scenes for r in s['robots']], np.int32)
    flags = d['idle'].astype(np.int32) | (d['lifting'].astype(np.int32) << 1)
    got_r = np.zeros(R, _lib.ROBOT_DTYPE)
    got_p = np.zeros((R * 2 * P, 2))
    rc = _lib.lib.simaps_pack_robots(R, d['pose'].ctypes.data, d['target'].ctypes.data, flags.ctypes.data,
                                     tg.ctypes.data, d['waypoints'].ctypes.data, d['waypoints'].shape[1],
                                     d['wp_count'].ctypes.data, d['wp_index'].ctypes.data, got_r.ctypes.data,
                                     got_p.ctypes.data)
    assert rc == 0, (rc, _lib.lib.simaps_last_error())
    for f in ('intention_len', 'history_len', 'group_index', 'type', 'idle', 'lifting'):
        assert np.array_equal(got_r[f], rob[f]), f
    assert max(rob['intention_len'].max(), rob['history_len'].max()) <= P
    for k in range(R):
        for f in ('intention', 'history'):
            n = rob[f + '_len'][k]
            assert paths[rob[f + '_off'][k]:][:n].tobytes() == got_p[got_r[f + '_off'][k]:][:n].tobytes(), (k, f)
    if name in D.FULL_CASES:
        f = scenes[0]['flags']
        if f['use_intention_map']:
            assert (rob['intention_len'] == P).all()
        if f['use_history_map']:
            assert (rob['history_len'] == P).all()


@pytest.mark.parametrize('name', SLOT_CASES)
def test_upper_slots_are_visible(name):
    """Agent 0 of every env: making robots 5.. idle (for spatial_5: robot 4) changes at least 50 pixels
    (10 for one robot) of every path channel of the oracle's stack, the last robot alone at least 10."""
    for e, s in enumerate(D.scenes(name)):
        nr = len(s['robots'])
        upper = tuple(k for k in range(5, nr) if not s['robots'][k]['idle']) or (nr - 1,)
        last = max(k for k in range(nr) if not s['robots'][k]['idle'])
        full = _state(name, e, 0)
        for c in D.path_channels(s['flags']):
            n_up = int((full[..., c] != _state(name, e, 0, upper)[..., c]).sum())
            n_last = int((full[..., c] != _state(name, e, 0, (last,))[..., c]).sum())
            print('%s env %d channel %d: robots %s %d px, robot %d %d px' % (name, e, c, list(upper), n_up, last, n_last))
            assert n_up >= (50 if len(upper) > 1 else 10), (name, e, c, n_up)
            assert n_last >= 10, (name, e, c, n_last)


def test_circle_targets_of_the_upper_robots_are_visible():
    """circle_8 fills no segment slot: each of robots 5, 6, 7 alone changes the intention channel (its
    target pixel lies inside agent 0's view)."""
    for e, s in enumerate(D.scenes('circle_8')):
        (c,) = D.path_channels(s['flags'])
        for k in (5, 6, 7):
            assert (_state('circle_8', e, 0)[..., c] != _state('circle_8', e, 0, (k,))[..., c]).any(), (e, k)


@pytest.mark.parametrize('name', ['ties_8', 'ties_8_spatial'])
def test_ties_are_exact(name):
    """Agent 0 sits on a pixel corner; at least two pairs of other robots are at bit-equal distance()
    from it and one other robot at distance 0; swapping two tied robots' channels would show."""
    for e, s in enumerate(D.scenes(name)):
        me = s['robots'][0]['position']
        H, W = s['H'], s['W']
        for v, n in ((me[0], W), (me[1], H)):
            assert float(v * 96 + n / 2).is_integer()
        dd = [O.distance(me, r['position']) for r in s['robots']]
        others = dd[1:]
        pairs = sum(others[i] == others[j] and others[i] > 0 for i in range(7) for j in range(i + 1, 7))
        assert pairs >= 2, dd
        assert sum(d == 0.0 for d in others) == 1
        order = sorted(range(8), key=lambda i: (dd[i], i))                 # ties in index order
        assert order != sorted(range(8), key=lambda i: (dd[i], -i))
        assert not any(r['idle'] for r in s['robots'])
        # the tied robots' channels differ, so their order is observable in the oracle's stack
        st = _state(name, e, 0)
        per = 1 if s['flags']['intention_channel_encoding'] == 'spatial' else 2
        c0 = st.shape[2] - per * 7
        chan = {k: st[..., c0 + per * q:c0 + per * (q + 1)] for q, k in enumerate(o for o in order if o != 0)}
        tied = [(i, j) for i in range(1, 8) for j in range(i + 1, 8) if dd[i] == dd[j]]
        assert any(not np.array_equal(chan[i], chan[j]) for i, j in tied)


def test_oracle_orders_tied_robots_by_index():
    """The reference orders the channels with np.argsort(dists) (envs.py:2353): numpy's insertion sort
    for 8 elements, so equal distances keep their index order -- but a numpy with a SIMD argsort
    (AVX-512, AVX2) breaks ties in another order, which differs between hosts.  The oracle's rule is
    the index order on every host (the kernel's too: intention_channel_order's insertion sort):
    channel q of every agent shows the target of the q-th other robot by (distance, index).  The
    scene_dense_ties_8 golden pins that rule to the reference, run without a SIMD argsort."""
    for s in D.scenes('ties_8_spatial'):
        scale = s['flags']['intention_map_scale']
        tied = 0
        for a in range(8):
            ao = O.AgentOracle(s, a)
            dd = [O.distance(s['robots'][a]['position'], r['position']) for r in s['robots']]
            tied += len(set(dd)) < 8
            others = [k for k in sorted(range(8), key=lambda i: (dd[i], i)) if k != a]
            chans = ao.intention_channels()
            assert len(chans) == 7
            for q, k in enumerate(others):
                gm = np.zeros(ao.shape, dtype=np.float32)
                t = s['robots'][k]['target_ee']
                gm[O.position_to_pixel_indices(t[0], t[1], ao.shape)] = scale
                assert np.array_equal(chans[q], ao._local_map(O.grey_dilation_cross(gm))), (a, q, k)
        assert tied == 8                     # robots 0 and 3 coincide: every agent sees at least that tie


def test_all_groups_show_their_segmentation_values():
    """all_8x4groups: the overhead channel of some agent holds 7/8 and 1.0 (robot groups 3 and 4)."""
    seen = set()
    for e in range(D.ENVS):
        for a in (0, 7):
            seen |= set(np.unique(_state('all_8x4groups', e, a)[..., 0]).tolist())
    assert {7 / 8, 1.0} <= seen, sorted(seen)
