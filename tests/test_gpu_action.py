"""GPU: device-side action decoding (include/simaps_action.h): the Q-map arg-max, Robot.store_new_action
(envs.py:857-903) on top of the unchanged movement path, the descriptor write-back, the context twin
and the Python layers, against the reference's own outputs (tests/golden/actions.npz) and the numpy
restatement tests/action_ref.py (pinned to that fixture by tests/test_action_abi.py).

Tolerances (fixture comparison and composition): waypoints the offset and back-up steps do not
touch are bit-equal; target, touched waypoints and source agree to 1e-12 m, headings to 1e-10 rad as an
angular difference.  The device and host libm may differ by an ulp in atan2 / cos / sin; coordinates
are below 4 m, where an ulp is 4e-16; the geometry chains about six operations; the shortest heading
segment of the fixture is 7e-3 m (1e-4 m by the generator's rule), so an ulp of a coordinate turns a
heading by at most ~1e-12 rad."""
import numpy as np
import pytest
import torch

import action_ref as A

pytestmark = pytest.mark.gpu

POS_TOL, HEAD_TOL = 1e-12, 1e-10
MIXED = 'lifting_2_pushing_2-large_empty-all'  # robots 0, 1 lifting (K = 2), robots 2, 3 pushing (K = 1)


@pytest.fixture(scope='module')
def S():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a GPU (run with -m gpu on an MI355X)')
    from simaps import _lib, batch, context, synthetic
    _lib.lib.simaps_fault_status(1)
    yield _lib, batch, context, synthetic
    torch.cuda.synchronize()
    _lib.lib.simaps_fault_status(1)


@pytest.fixture(params=[1, 2, 3], ids=['compact', 'early_exit', 'overlap'])
def path_mode(request):
    """Every path kernel variant (include/simaps.h simaps_path_mode), as in tests/test_gpu_dropin.py."""
    from simaps import _lib
    prev = _lib.lib.simaps_path_mode(request.param)
    yield request.param
    _lib.lib.simaps_path_mode(prev)


_BATCHES = {}


def _fixture_batch(S, config):
    """One StateBatch over the two scenes a config's fixture cases were drawn on (built once)."""
    _lib, batch, context, synthetic = S
    if config not in _BATCHES:
        seeds = sorted({c['seed'] for c in A.load_cases() if c['config'] == config})
        scenes = [A.make_scene(synthetic, config, s) for s in seeds]
        _BATCHES[config] = (batch.StateBatch(scenes), seeds)
    return _BATCHES[config]


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _check_case(c, h, n, wp_key='wp', hd_key='hd', source=None):
    """Agent n of a downloaded result against fixture case c (or a dict of the same keys)."""
    want_wp, want_hd = c[wp_key], c[hd_key]
    cnt = int(h['count'][n])
    assert int(h['action'][n]) == c['action']
    a = int(h['action'][n])
    assert (a // 9216, a % 9216 // 96, a % 96) == tuple(c['tuple'])
    assert cnt == len(want_wp), (cnt, len(want_wp))
    got_wp, got_hd = h['xy'][n, :cnt], h['heading'][n, :cnt]
    backup = cnt > 2 and wp_key == 'wp' and not np.array_equal(c['path'][-2], c['wp'][-2])
    touched = {cnt - 1} | ({cnt - 2} if backup else set())
    for k in range(cnt):
        if k in touched:
            assert np.abs(got_wp[k] - want_wp[k]).max() <= POS_TOL, (k, got_wp[k], want_wp[k])
        else:  # the source and the pixel-centre waypoints
            assert np.array_equal(_bits(got_wp[k]), _bits(want_wp[k])), (k, got_wp[k], want_wp[k])
    assert np.abs(h['target'][n] - c['target']).max() <= POS_TOL
    assert np.abs(h['source'][n] - (want_wp[0] if source is None else source)).max() <= POS_TOL
    assert A.angle_diff(got_hd, want_hd).max() <= HEAD_TOL, (got_hd, want_hd)


# ---- 1. arg-max ----------------------------------------------------------------------------------
# The decode kernel's striping (csrc/action.h): a 16-byte-aligned block is read in float4 groups,
# group g = i // 4 by thread g % NT (wave (g % NT) // 64) as that thread's (g // NT)-th group; any
# other block one float at a time, element i by thread i % NT.
NT = 768  # ACT_NT
def _argmax_blocks(T, rs):
    """name -> [T] float32 block.  Noise in (-1, 1); planted maxima are 5."""
    def noise():
        return rs.uniform(-1, 1, T).astype(np.float32)
    out = {}
    for name, idx in (('max_at_0', [0]), ('max_at_last', [T - 1]), ('first_of_group', [4 * 777]), ('last_of_group', [4 * 777 + 3]),
                      # equal maxima, the LATER one held by a lower-numbered wave: group 200 (thread 200,
                      # wave 3) before group NT + 5 (thread 5, wave 0)
                      ('tie_lower_wave', [4 * 200 + 1, 4 * (NT + 5) + 2]),
                      # ... by a lower lane of the same wave: thread 40 before thread 3 (wave 0)
                      ('tie_lower_lane', [4 * 40, 4 * (NT + 3)]),
                      # ... inside one thread's own sequence and one 16-byte group
                      ('tie_same_thread', [4 * 9 + 1, 4 * 9 + 2, 4 * (2 * NT + 9)]),
                      # ... for the 4-byte path: element 200 (thread 200) before element NT + 5 (thread 5)
                      ('tie_scalar_striping', [200, NT + 5])):
        b = noise()
        b[idx] = 5.0
        out[name] = b
    out['constant'] = np.full(T, 0.25, np.float32)
    out['all_neg_inf'] = np.full(T, -np.inf, np.float32)
    b = noise()
    b[4 * 300 + 2] = np.nan                                   # one NaN, with greater finite values before it
    b[17] = 5.0
    out['one_nan'] = b
    b = noise()
    b[[4 * 250 + 3, 4 * (NT + 1)]] = np.nan                   # two NaNs, the later one on a lower thread
    out['two_nans'] = b
    b = np.full(T, -0.0, np.float32)
    b[5] = 0.0                                                # -0.0 == +0.0: index 0 stays the arg-max
    out['neg_zero_first'] = b
    b = np.full(T, -1.0, np.float32)
    b[4 * 130] = 0.0
    b[4 * (NT + 2)] = -0.0                                    # +0.0 first, -0.0 later on a lower thread
    b[T - 1] = 0.0
    out['pos_zero_first'] = b
    return out


def _np_argmax(block):
    return int(np.argmax(np.where(np.isnan(block), np.inf, block)))


@pytest.mark.parametrize('shift', [0, 1, 2, 3], ids=['aligned', 'off1', 'off2', 'off3'])
def test_argmax_corner_cases(S, shift):
    """Exact against np.argmax (NaN as +inf) for K = 2, K = 1 and K = 2 agents in one launch (N = 3),
    blocks packed back to back with gaps.  shift != 0: every q_off is 4 m + shift floats, which the
    kernel accepts (4-byte loads)."""
    _lib, batch, context, synthetic = S
    b = batch.StateBatch([synthetic.make_scene(MIXED, 0)])
    slots, Ts = [0, 2, 1], [2 * 9216, 9216, 2 * 9216]
    rs = np.random.RandomState(11 + shift)
    blocks = [_argmax_blocks(T, rs) for T in Ts]
    names = sorted(blocks[0])
    offs = np.array([8 + shift, 8 + Ts[0] + 12 + shift, 8 + Ts[0] + 12 + Ts[1] + 4 + shift], dtype=np.int64)
    total = int(offs[2] + Ts[2] + 8)
    for k, name in enumerate(names):
        flat = np.full(total, 9.0, np.float32)                # (greater than every planted maximum: a read
        picks = [names[(k + j) % len(names)] for j in range(3)]  # outside a block would win)
        for o, T, bl, p in zip(offs, Ts, blocks, picks):
            flat[o:o + T] = bl[p]
        r = b.store_new_actions(q=torch.from_numpy(flat).to(b.device), q_off=offs, slots=slots,
                                use_shortest_path_movement=False, max_points=2)
        h = r.to_host()
        want = [_np_argmax(bl[p]) for bl, p in zip(blocks, picks)]
        assert h['action'].tolist() == want, (picks, h['action'].tolist(), want)
        assert h['count'].tolist() == [2, 2, 2]
    _lib.check_faults()


# ---- 2. actions_in -------------------------------------------------------------------------------
def test_actions_override_and_mixing(S):
    _lib, batch, context, synthetic = S
    b = batch.StateBatch([synthetic.make_scene(MIXED, 1)])
    slots = [0, 1, 2, 3]
    rs = np.random.RandomState(5)
    q = [torch.from_numpy(rs.uniform(-1, 1, (2, k, 96, 96)).astype(np.float32)).to(b.device) for k in (2, 1)]
    greedy = [int(t[i].reshape(-1).argmax()) for t in q for i in range(2)]
    groups = [(q[0], [0, 1]), (q[1], [2, 3])]
    h = b.store_new_actions(q=groups, slots=slots, use_shortest_path_movement=False).to_host()
    assert h['action'].tolist() == greedy
    mixed = [-1, 18431, 9215, -1]                             # given indices are used as they are
    h2 = b.store_new_actions(q=groups, actions=mixed, slots=slots, use_shortest_path_movement=False).to_host()
    assert h2['action'].tolist() == [greedy[0], 18431, 9215, greedy[3]]
    given = [0, 12345, 9215, 4000]                            # no q at all
    h3 = b.store_new_actions(actions=given, slots=slots, use_shortest_path_movement=False).to_host()
    assert h3['action'].tolist() == given
    for n, a in enumerate(given):                             # and the geometry follows the chosen index
        r = b.scenes[0]['robots'][n]
        t = A.target(a, A.TYPE_IDS[r['type']], r['position'], r['heading'])
        assert np.abs(h3['target'][n] - np.asarray(t)).max() <= POS_TOL
        assert np.array_equal(_bits(h3['source'][n]), _bits(np.asarray(r['position'][:2], dtype=np.float64)))
    with pytest.raises(ValueError):
        b.store_new_actions(slots=slots)
    _lib.check_faults()


# ---- 3. / 4. the reference's own outputs ------------------------------------------------------------
CONFIGS = sorted({c['config'] for c in A.load_cases()})


@pytest.mark.parametrize('config', CONFIGS)
def test_reference_goldens(S, path_mode, config):
    """Every fixture case of a config through the ABI (explicit actions), 64 agents per launch."""
    _lib, batch, context, synthetic = S
    b, seeds = _fixture_batch(S, config)
    slot = {ea: n for n, ea in enumerate(b.agents)}
    cases = [c for c in A.load_cases() if c['config'] == config]
    for k0 in range(0, len(cases), 64):
        chunk = cases[k0:k0 + 64]
        slots = [slot[(seeds.index(c['seed']), c['agent'])] for c in chunk]
        h = b.store_new_actions(actions=[c['action'] for c in chunk], slots=slots, max_points=16).to_host()
        for n, c in enumerate(chunk):
            _check_case(c, h, n)
    _lib.check_faults()


def test_shortest_path_movement_off(S):
    _lib, batch, context, synthetic = S
    seen = 0
    for config in CONFIGS:
        b, seeds = _fixture_batch(S, config)
        slot = {ea: n for n, ea in enumerate(b.agents)}
        chunk = [c for c in A.load_cases() if c['config'] == config and 'wp_nospm' in c]
        slots = [slot[(seeds.index(c['seed']), c['agent'])] for c in chunk]
        h = b.store_new_actions(actions=[c['action'] for c in chunk], slots=slots, max_points=4,
                                use_shortest_path_movement=False).to_host()
        for n, c in enumerate(chunk):
            _check_case(c, h, n, 'wp_nospm', 'hd_nospm')
        seen += len(chunk)
    assert seen >= 21
    _lib.check_faults()


# ---- 5. composition -------------------------------------------------------------------------------
@pytest.mark.parametrize('config,observe_all', [('lifting_4-small_divider', False), ('lifting_4-large_doors', True),
                                                (MIXED, False)])
def test_composition_on_fresh_scenes(S, config, observe_all):
    """Greedy actions from random Q maps on scenes no fixture holds: the waypoints before the offset
    are StateBatch.shortest_paths(out_source, out_target) bit for bit, the rest is action_ref on them."""
    _lib, batch, context, synthetic = S
    scenes = [synthetic.make_scene(config, 900 + e, observe_all=observe_all) for e in range(4)]
    b = batch.StateBatch(scenes)
    types = [A.TYPE_IDS[scenes[e]['robots'][a]['type']] for e, a in b.agents]
    g = torch.Generator().manual_seed(3)
    blocks = [torch.randn(A.NUM_OUTPUT_CHANNELS[t], 96, 96, generator=g) for t in types]
    off = np.cumsum([0] + [bl.numel() for bl in blocks[:-1]]).astype(np.int64)
    q = torch.cat([bl.reshape(-1) for bl in blocks]).to(b.device)
    h = b.store_new_actions(q=q, q_off=off, max_points=16).to_host()
    paths = b.shortest_paths(h['source'], h['target'], max_points=16)
    detours = 0
    for n, (e, a) in enumerate(b.agents):
        r = scenes[e]['robots'][a]
        act = int(blocks[n].reshape(-1).argmax())
        pre = np.array([p[:2] for p in paths[n]], dtype=np.float64)
        assert np.array_equal(_bits(pre[-1]), _bits(h['target'][n]))
        wp, hd, sd = A.finish(pre, types[n], r['heading'])
        want = {'action': act, 'tuple': A.action_tuple(act, types[n]), 'path': pre, 'wp': wp, 'hd': hd,
                'target': np.asarray(A.target(act, types[n], r['position'], r['heading']))}
        _check_case(want, h, n)
        assert np.array_equal(_bits(h['source'][n]), _bits(np.asarray(r['position'][:2], dtype=np.float64)))
        detours += len(pre) > 2
    if config != MIXED:
        assert detours >= 1                                   # (the empty room has only straight paths)
    _lib.check_faults()


# ---- 6. write-back ---------------------------------------------------------------------------------
@pytest.mark.parametrize('config', ['lifting_4-small_divider', 'lifting_4-small_divider-history'])
def test_write_back_equals_a_host_repack(S, config):
    _lib, batch, context, synthetic = S
    scenes = [synthetic.make_scene(config, 920 + e) for e in range(3)]
    b = batch.StateBatch(scenes)
    arr = batch.descriptor_arrays(scenes)
    P = _lib.MAX_PATH
    wps = np.zeros((b.n_robots, P, 2))
    wps[:, :arr['waypoints'].shape[1]] = arr['waypoints']
    arr['waypoints'] = wps
    with pytest.raises(ValueError, match='set_descriptor_arrays'):
        b.store_new_actions(actions=[0] * b.N, write_back=True)  # set_descriptors() layout: refused
    b.set_descriptor_arrays(**arr)
    before_r = b.robots_d.cpu().numpy().view(_lib.ROBOT_DTYPE)
    before_p = b.paths_d.cpu().numpy().view(np.int64).reshape(b.n_robots, 2 * P, 2)
    acting = [1, 2, 4, 7, 8, 11]                              # slot n is robot n here (every agent, in order)
    assert [e * 4 + a for e, a in b.agents] == list(range(b.N))
    g = torch.Generator().manual_seed(8)
    q = torch.randn(len(acting), 2, 96, 96, generator=g).to(b.device)
    res = b.store_new_actions(q=q, slots=acting, max_points=P, write_back=True)
    state1 = b.render().clone()
    after_r = b.robots_d.cpu().numpy().view(_lib.ROBOT_DTYPE).copy()
    after_p = b.paths_d.cpu().numpy().view(np.int64).reshape(b.n_robots, 2 * P, 2).copy()
    h = res.to_host()
    assert (h['count'] >= 2).all() and (h['count'] <= P).all()
    # the host route: the same values through simaps_pack_robots (wp_index 1, idle 0, the new target)
    for n, r in enumerate(acting):
        c = int(h['count'][n])
        arr['target'][r] = h['target'][n]
        arr['idle'][r] = False
        arr['waypoints'][r] = 0
        arr['waypoints'][r, :c] = h['xy'][n, :c]
        arr['wp_count'][r] = c
        arr['wp_index'][r] = 1
    b.set_descriptor_arrays(**arr)
    packed_r = b.robots_d.cpu().numpy().view(_lib.ROBOT_DTYPE)
    packed_p = b.paths_d.cpu().numpy().view(np.int64).reshape(b.n_robots, 2 * P, 2)
    state2 = b.render()
    assert torch.equal(state1.view(torch.int32), state2.view(torch.int32))
    for r in range(b.n_robots):
        if r in acting:
            assert after_r[r].tobytes() == packed_r[r].tobytes(), r   # ints equal, doubles bit-equal
            il, hl = int(after_r[r]['intention_len']), int(after_r[r]['history_len'])
            assert il == int(h['count'][acting.index(r)]) and hl == 2 and after_r[r]['idle'] == 0
            assert np.array_equal(after_p[r, :il], packed_p[r, :il])
            assert np.array_equal(after_p[r, P:P + hl], packed_p[r, P:P + hl])
        else:                                                  # robots that did not act: untouched
            assert after_r[r].tobytes() == before_r[r].tobytes(), r
            assert np.array_equal(after_p[r], before_p[r]), r
    _lib.check_faults()


# ---- 7. / 8. contexts ------------------------------------------------------------------------------
@pytest.fixture
def AB(S):
    _lib, batch, context, synthetic = S
    a, b = context.Context(), context.Context()
    yield a, b
    torch.cuda.synchronize()
    for c in (a, b):
        if c._open:
            c.fault_status(clear=True)
        c.close()
    _lib.lib.simaps_fault_status(1)


def _small_divider_run(S, ctx, actions=None, **kw):
    _lib, batch, context, synthetic = S
    scenes = [synthetic.make_scene('lifting_4-small_divider', 60 + e) for e in range(2)]
    b = batch.StateBatch(scenes, context=ctx)
    g = torch.Generator().manual_seed(21)
    q = torch.randn(b.N, 2, 96, 96, generator=g).to(b.device)
    return b, q, b.store_new_actions(q=q, actions=actions, max_points=16, **kw)


def test_context_twin_is_bitwise_the_plain_call(S, AB):
    a, b2 = AB
    want = _small_divider_run(S, None)[2].to_host()
    for ctx in (a, b2):
        got = _small_divider_run(S, ctx)[2].to_host()
        for k in ('action', 'source', 'target', 'count'):
            assert got[k].tobytes() == want[k].tobytes(), k
        for n, c in enumerate(want['count']):
            assert got['xy'][n, :c].tobytes() == want['xy'][n, :c].tobytes()
            assert got['heading'][n, :c].tobytes() == want['heading'][n, :c].tobytes()
        assert ctx.fault_info() == (0, None, None)
    assert (want['count'] > 2).any()


def test_bad_action_is_reported_to_its_context_only(S, AB):
    """The fault record is a status word: the decode kernel posts SIMAPS_FAULT_DESCRIPTOR with its
    kernel id and the agent index, skips that agent, and finishes the others."""
    _lib, batch, context, synthetic = S
    a, b2 = AB
    want = _small_divider_run(S, None)[2].to_host()
    actions = [-1] * 8
    actions[5] = 2 * 9216                                     # one past the last index of a K = 2 robot
    ba, qa, res = _small_divider_run(S, a, actions=actions)
    got = res.to_host()                                       # (synchronises)
    assert got['count'][5] == 0
    for n in range(8):
        if n != 5:
            c = int(want['count'][n])
            assert got['count'][n] == c and got['action'][n] == want['action'][n]
            assert got['xy'][n, :c].tobytes() == want['xy'][n, :c].tobytes()
            assert got['heading'][n, :c].tobytes() == want['heading'][n, :c].tobytes()
    assert a.fault_info() == (_lib.FAULT_DESCRIPTOR, 'action', 5)
    assert b2.fault_info() == (0, None, None)
    with pytest.raises(_lib.DeviceFault, match='in action, unit 5'):   # A's next call: SIMAPS_EDEVICE, once
        ba.store_new_actions(q=qa, max_points=16)
    assert ba.store_new_actions(q=qa, max_points=16).to_host()['count'].tolist() == want['count'].tolist()
    assert _small_divider_run(S, b2)[2].to_host()['count'].tolist() == want['count'].tolist()
    assert _lib.lib.simaps_fault_status(0) == 0              # nor the default context


# ---- 9. small buffer -------------------------------------------------------------------------------
def test_small_buffer_reports_the_needed_count(S):
    _lib, batch, context, synthetic = S
    config = 'lifting_4-large_doors'
    b, seeds = _fixture_batch(S, config)
    slot = {ea: n for n, ea in enumerate(b.agents)}
    cases = [c for c in A.load_cases() if c['config'] == config]
    long = next(c for c in cases if len(c['wp']) >= 5)
    short = [c for c in cases if len(c['wp']) <= 3][:3]
    chunk = [short[0], long] + short[1:]
    slots = [slot[(seeds.index(c['seed']), c['agent'])] for c in chunk]
    h = b.store_new_actions(actions=[c['action'] for c in chunk], slots=slots, max_points=3).to_host()
    assert h['count'][1] == -len(long['wp'])
    for n, c in enumerate(chunk):
        if n != 1:
            _check_case(c, h, n)
    _lib.check_faults()


# ---- 10. drop-in level -----------------------------------------------------------------------------
def test_vector_env_store_new_action(S):
    """VectorEnv.store_new_action's [group][robot] -> index or None structure, per env; one env from
    explicit indices, the other greedy from policy outputs with the fixture's action as the maximum."""
    _lib, batch, context, synthetic = S
    from simaps import vector_env
    config = 'lifting_4-small_divider'
    seeds = [60, 61]
    scenes = [A.make_scene(synthetic, config, s) for s in seeds]
    obs = vector_env.VectorEnvObservations(scenes, layout='chw')
    pick = {}
    for c in A.load_cases():
        if c['config'] == config and len(c['wp']) > 2:
            pick.setdefault((seeds.index(c['seed']), c['agent']), c)
    assert len(pick) >= 5
    pick.pop(sorted(pick)[1])                                 # one robot of env 0 does not act
    action = [[[pick[(0, a)]['action'] if (0, a) in pick else None for a in range(4)]], [[None] * 4]]
    idx = [a for a in range(4) if (1, a) in pick]
    q = torch.zeros(len(idx), 2, 96, 96)
    for i, a in enumerate(idx):
        q[i].view(-1)[pick[(1, a)]['action']] = 1.0
    outputs = [[([], None)], [(idx, q.to(obs.batch.device))]]
    got = obs.store_new_action(action, outputs=outputs, max_points=16)
    assert [len(g) for e in got for g in e] == [4, 4]
    for e in range(2):
        for a in range(4):
            r = got[e][0][a]
            if (e, a) not in pick:
                assert r is None
                continue
            c = pick[(e, a)]
            assert r['action'] == c['tuple'] and isinstance(r['action'], tuple)
            assert len(r['target_end_effector_position']) == 3 and r['target_end_effector_position'][2] == 0
            h = {'action': np.array([c['action']]), 'count': np.array([len(r['waypoint_positions'])]),
                 'xy': np.array([[p[:2] for p in r['waypoint_positions']]]),
                 'heading': np.array([r['waypoint_headings']]),
                 'target': np.array([r['target_end_effector_position'][:2]]),
                 'source': np.array([r['waypoint_positions'][0][:2]])}
            _check_case(c, h, 0)
            assert all(len(p) == 3 and p[2] == 0 for p in r['waypoint_positions'])
    assert obs.store_new_action([[[None] * 4]] * 2) == [[[None] * 4]] * 2          # nobody acts: no launch
