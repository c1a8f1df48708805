"""GPU: simaps_store_new_action_as (include/simaps_action_as.h): float32 against the older entry point
bit for bit, the arg-max of bf16 / fp16 Q maps against np.argmax of the widened block, the
exploration draw against its restatement tests/explore_ref.py (pinned to the published Philox known
answers by tests/test_action_as_abi.py), the rng state under graph replay, a bad eps as a contained
descriptor error, and the Python layers.

Everything compared here is exact: integers, or float64 outputs of the same device code."""

import numpy as np
import pytest
import torch

import action_ref as A
import explore_ref as E

pytestmark = pytest.mark.gpu

DIVIDER = 'lifting_4-small_divider'                 # four lifting robots: K = 2, total 18,432
MIXED = 'lifting_2_pushing_2-large_empty-all'       # robots 0, 1 lifting (K = 2), robots 2, 3 pushing (K = 1)
DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16}


@pytest.fixture(scope='module')
def S():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a GPU (run with -m gpu on an MI355X)')
    from simaps import _lib, batch, context, synthetic
    _lib.lib.simaps_fault_status(1)
    yield _lib, batch, context, synthetic
    torch.cuda.synchronize()
    _lib.lib.simaps_fault_status(1)


def _np_argmax(block):
    return int(np.argmax(np.where(np.isnan(block), np.inf, block)))


def _with_array_descriptors(S, b, scenes):
    """The descriptor layout the write-back needs (as tests/test_gpu_action.py makes it)."""
    _lib, batch, context, synthetic = S
    arr = batch.descriptor_arrays(scenes)
    wps = np.zeros((b.n_robots, _lib.MAX_PATH, 2))
    wps[:, :arr['waypoints'].shape[1]] = arr['waypoints']
    arr['waypoints'] = wps
    b.set_descriptor_arrays(**arr)
    return arr


# ---- 1. float32 without exploration is the older entry point ------------------------------------------
def _raw(S, b, name, q, q_off, flags, max_points, extra):
    """One of the two entry points on all agents of b, outputs pre-filled so that whole tensors compare."""
    _lib = S[0]
    n = b.N
    out = [torch.full((n,), -7, dtype=torch.int32, device=b.device), torch.zeros((n, 2), dtype=torch.float64, device=b.device),
           torch.zeros((n, 2), dtype=torch.float64, device=b.device),
           torch.zeros((n, max_points, 2), dtype=torch.float64, device=b.device),
           torch.zeros((n, max_points), dtype=torch.float64, device=b.device),
           torch.full((n,), -7, dtype=torch.int32, device=b.device)]
    head = [b.cfg, n, _lib.ptr(b.agents_d), _lib.ptr(b.envs_d), _lib.ptr(b.robots_d), _lib.ptr(b.paths_d),
            _lib.ptr(b.occupancy), _lib.ptr(q)]
    if name == 'store_new_action':
        args = head + [_lib.ptr(q_off), None, flags, max_points] + [_lib.ptr(t) for t in out] + [_lib.stream_handle()]
    else:
        args = head + [_lib.STATE_F32, _lib.ptr(q_off), None] + extra + [flags, max_points] + [_lib.ptr(t) for t in out] + \
            [None, _lib.stream_handle()]
    _lib.check(_lib.call(b.context, name, *args))
    torch.cuda.synchronize()
    return out


def _defined_paths(_lib, b):
    """paths_d with everything past each robot's intention_len / history_len points zeroed (the
    staging buffer behind it is not initialised there)."""
    P = _lib.MAX_PATH
    rob = b.robots_d.cpu().numpy().view(_lib.ROBOT_DTYPE)
    pts = b.paths_d.cpu().numpy().view(np.int64).reshape(b.n_robots, 2 * P, 2).copy()
    for r in range(b.n_robots):
        pts[r, min(int(rob[r]['intention_len']), P):P] = 0
        pts[r, P + min(int(rob[r]['history_len']), P):] = 0
    return torch.from_numpy(pts)


@pytest.mark.parametrize('spm', [False, True], ids=['straight', 'shortest_path'])
@pytest.mark.parametrize('wb', [False, True], ids=['no_write_back', 'write_back'])
def test_float32_without_eps_equals_the_older_entry_point(S, spm, wb):
    _lib, batch, context, synthetic = S
    scenes = [synthetic.make_scene(DIVIDER, 60 + e) for e in range(2)]
    b = batch.StateBatch(scenes)
    g = torch.Generator().manual_seed(21)
    q = torch.randn(b.N, 2, 96, 96, generator=g).to(b.device)
    q_off = torch.arange(b.N, dtype=torch.int64, device=b.device) * 18432
    flags = (_lib.ACTION_SHORTEST_PATH if spm else 0) | (_lib.ACTION_WRITE_BACK if wb else 0)
    got = {}
    for name in ('store_new_action', 'store_new_action_as'):
        _with_array_descriptors(S, b, scenes)                   # (a write-back changes them: fresh for each call)
        out = _raw(S, b, name, q, q_off, flags, _lib.MAX_PATH, [None, None])
        got[name] = out + [b.robots_d.clone(), _defined_paths(_lib, b)]
    for k, (x, y) in enumerate(zip(got['store_new_action'], got['store_new_action_as'])):
        assert torch.equal(x, y), k
    cnt = got['store_new_action'][5]
    assert (cnt >= 2).all() and ((cnt > 2).any() if spm else (cnt == 2).all())
    _lib.check_faults()


# ---- 2. the 16-bit arg-max ------------------------------------------------------------------------------
# The 16-bit decode kernels' striping (csrc/simaps_action_as.hip): a 16-byte-aligned block is read in
# groups of 8 elements, group g = i // 8 by thread g % NT16 (wave (g % NT16) // 64) as that thread's
# (g // NT16)-th group -- all of a thread's groups in one round of loads; a K = 1 block has one and a
# half groups per thread, the second one on threads below NT16 / 2.  Any other block is read one
# element at a time, element i by thread i % NT16.
NT16 = 768


def _argmax_blocks(T, rs, dtype):
    """name -> [T] block of `dtype` (a torch tensor).  Noise in (-1, 1) rounded to the dtype; planted maxima are 5."""
    def noise():
        return rs.uniform(-1, 1, T).astype(np.float32)
    out = {'noise': noise()}                                      # its maximum is then often there twice
    planted = [('max_at_0', [0]), ('max_at_last', [T - 1]), ('group_edge_7', [7]), ('group_edge_8', [8]),
               ('channel_edge_9215', [min(9215, T - 1)]), ('channel_edge_9216', [9216 % T]),
               # equal maxima, 16-byte path: the lower index in group 200 (thread 200), the higher in group
               # NT16 + 5 (thread 5, wave 0) -- and the reverse
               ('tie_group_low_on_high_thread', [8 * 200 + 1, 8 * (NT16 + 5) + 2]),
               ('tie_group_low_on_low_thread', [8 * 5 + 6, 8 * (NT16 + 200) + 3]),
               # the same for the element path: element 200 (thread 200) before NT16 + 5 (thread 5), and the reverse
               ('tie_elem_low_on_high_thread', [200, NT16 + 5]),
               ('tie_elem_low_on_low_thread', [5, NT16 + 200])]
    for name, idx in planted:
        b = noise()
        b[idx] = 5.0
        out[name] = b
    out['constant'] = np.full(T, 0.25, np.float32)
    out['all_neg_inf'] = np.full(T, -np.inf, np.float32)
    b = noise()
    b[17] = 5.0
    b[8 * 300 + 2] = np.inf                                       # +inf (fp16's too) behind a finite maximum
    out['pos_inf'] = b
    b = noise()
    b[8 * 300 + 2] = np.nan                                       # one NaN, with greater finite values before it
    b[17] = 5.0
    out['one_nan'] = b
    b = noise()
    b[[8 * 250 + 3, 8 * (NT16 + 1)]] = np.nan                     # two NaNs, the later one on a lower thread
    out['two_nans'] = b
    b = np.full(T, -1.0, np.float32)
    b[8 * 130] = -0.0
    b[8 * (NT16 + 2)] = 0.0                                       # -0.0 low, +0.0 high (on a lower thread)
    out['neg_zero_low'] = b
    b = np.full(T, -1.0, np.float32)
    b[8 * 130] = 0.0
    b[8 * (NT16 + 2)] = -0.0                                      # and the reverse
    b[T - 1] = 0.0
    out['pos_zero_low'] = b
    return {k: torch.from_numpy(v).to(dtype) for k, v in out.items()}


@pytest.mark.parametrize('shift', [0, 1, 4], ids=['aligned', 'off1', 'off4'])
@pytest.mark.parametrize('dt', sorted(DTYPES))
def test_argmax_16bit_corner_cases(S, dt, shift):
    """Exact against np.argmax (NaN as +inf) of the block widened to float32, for K = 2, K = 1 and K = 2
    agents in one launch (N = 3), blocks packed with gaps into a buffer of a value above every
    planted maximum.  shift: every q_off is 8 m + shift elements (0: 16-byte loads; 1, 4: element loads)."""
    _lib, batch, context, synthetic = S
    dtype = DTYPES[dt]
    b = batch.StateBatch([synthetic.make_scene(MIXED, 0)])
    slots, Ts = [0, 2, 1], [2 * 9216, 9216, 2 * 9216]
    rs = np.random.RandomState(11 + shift)
    blocks = [_argmax_blocks(T, rs, dtype) for T in Ts]
    wide = [{k: v.float().numpy() for k, v in bl.items()} for bl in blocks]
    names = sorted(blocks[0])
    offs = np.array([8 + shift, 8 + Ts[0] + 16 + shift, 8 + Ts[0] + 16 + Ts[1] + 8 + shift], dtype=np.int64)
    total = int(offs[2] + Ts[2] + 8)
    base = torch.full((total,), 9.0, dtype=dtype, device=b.device)   # (greater than every planted finite maximum:
    assert base.data_ptr() % 16 == 0                                 # a read outside a block would win)
    for k, name in enumerate(names):
        flat = base.clone()
        picks = [names[(k + j) % len(names)] for j in range(3)]
        for o, T, bl, p in zip(offs, Ts, blocks, picks):
            flat[o:o + T] = bl[p].to(b.device)
        r = b.store_new_actions(q=flat, q_off=offs, slots=slots, use_shortest_path_movement=False, max_points=2)
        h = r.to_host()
        want = [_np_argmax(w[p]) for w, p in zip(wide, picks)]
        assert h['action'].tolist() == want, (picks, h['action'].tolist(), want)
        assert h['count'].tolist() == [2, 2, 2]
        assert h['explored'] is None
    _lib.check_faults()


# ---- 3. precedence ------------------------------------------------------------------------------------------
def test_given_beats_drawn_beats_argmax(S):
    _lib, batch, context, synthetic = S
    from simaps import policy_output
    b = batch.StateBatch([synthetic.make_scene(MIXED, 1)])
    totals = [18432, 18432, 9216, 9216]
    nan = [(torch.full((2, k, 96, 96), float('nan'), dtype=torch.bfloat16, device=b.device), pos)
           for k, pos in ((2, [0, 1]), (1, [2, 3]))]            # an agent that read its block would answer 0
    rng = policy_output.DeviceExploration(77, b.device, step=5)
    given = [-1, 100, -1, 9000]
    h = b.store_new_actions(q=nan, actions=given, use_shortest_path_movement=False, max_points=2, exploration_eps=1.0,
                            rng=rng).to_host()
    ex, act = E.draws(77, 5, 4, 1.0, totals)
    assert ex.all()
    assert h['explored'].tolist() == [1, 0, 1, 0]
    assert h['action'].tolist() == [int(act[0]), 100, int(act[2]), 9000]
    assert act[0] != 0 and act[2] != 0
    assert h['count'].tolist() == [2, 2, 2, 2]
    # eps 0: nobody draws; with a real block the -1 agents take the arg-max
    g = torch.Generator().manual_seed(2)
    q = [(torch.randn(2, k, 96, 96, generator=g).to(torch.float16).to(b.device), pos) for k, pos in ((2, [0, 1]), (1, [2, 3]))]
    h0 = b.store_new_actions(q=q, actions=given, use_shortest_path_movement=False, max_points=2, exploration_eps=0.0,
                             rng=rng).to_host()
    assert h0['explored'].tolist() == [0, 0, 0, 0]
    assert h0['action'].tolist() == [_np_argmax(q[0][0][0].float().cpu().numpy().reshape(-1)), 100,
                                     _np_argmax(q[1][0][0].float().cpu().numpy().reshape(-1)), 9000]
    # no q at all: every agent given or drawn is fine
    h1 = b.store_new_actions(actions=given, use_shortest_path_movement=False, max_points=2, exploration_eps=1.0,
                             rng=rng).to_host()
    ex7, act7 = E.draws(77, 7, 4, 1.0, totals)
    assert h1['action'].tolist() == [int(act7[0]), 100, int(act7[2]), 9000]
    assert rng.step == 8
    _lib.check_faults()


# ---- 4. the draw is the stated function ------------------------------------------------------------------
@pytest.fixture(scope='module')
def BIG(S):
    """64 envs x 4 agents of lifting_4-small_divider (four distinct scenes, sixteen times), a bf16 Q
    block per agent and its arg-max on the host, computed once."""
    _lib, batch, context, synthetic = S
    four = [synthetic.make_scene(DIVIDER, 300 + e) for e in range(4)]
    b = batch.StateBatch([four[e % 4] for e in range(64)])
    assert b.N == 256
    g = torch.Generator().manual_seed(31)
    q = torch.randn(256, 2, 96, 96, generator=g).to(torch.bfloat16)
    greedy = np.array([_np_argmax(row) for row in q.float().numpy().reshape(256, -1)])
    return b, q.to(b.device), greedy


def test_draw_equals_the_restatement_over_16_steps(S, BIG):
    _lib, batch, context, synthetic = S
    from simaps import policy_output
    b, q, greedy = BIG
    want = [E.draws(1234, step, 256, 0.25, 18432) for step in range(7, 23)]
    assert sum(int(ex.sum()) for ex, _ in want) == 1059          # the restatement alone, on exactly these inputs
    rng = policy_output.DeviceExploration(1234, b.device, step=7)
    res = [b.store_new_actions(q=q, use_shortest_path_movement=False, max_points=2, exploration_eps=0.25, rng=rng)
           for _ in range(16)]
    for (ex, act), r in zip(want, res):
        h = r.to_host()
        assert 0 < ex.sum() < 256                                 # explored and greedy agents in every call
        assert np.array_equal(h['explored'].astype(bool), ex)
        assert np.array_equal(h['action'], np.where(ex, act, greedy))
        assert (h['count'] == 2).all()
    assert rng.step == 23
    # another seed: another pattern
    rng2 = policy_output.DeviceExploration(4321, b.device, step=7)
    h2 = b.store_new_actions(q=q, use_shortest_path_movement=False, max_points=2, exploration_eps=0.25, rng=rng2).to_host()
    ex2, act2 = E.draws(4321, 7, 256, 0.25, 18432)
    assert np.array_equal(h2['explored'].astype(bool), ex2) and not np.array_equal(ex2, want[0][0])
    assert np.array_equal(h2['action'], np.where(ex2, act2, greedy))
    _lib.check_faults()


def test_subset_launch_draws_by_the_calls_agent_index(S, BIG):
    _lib, batch, context, synthetic = S
    from simaps import policy_output
    b, q, greedy = BIG
    slots = [200, 5, 17, 3, 254, 100, 64, 9]
    rng = policy_output.DeviceExploration(1234, b.device, step=7)
    eps = np.array([0.5, 1.0, 0.0, 0.5, 0.5, 1.0, 0.5, 0.5], dtype=np.float32)   # (per agent, as an array)
    h = b.store_new_actions(q=q[slots], slots=slots, use_shortest_path_movement=False, max_points=2,
                            exploration_eps=eps, rng=rng).to_host()
    ex, act = E.draws(1234, 7, len(slots), eps, 18432)           # n = the position in the call, not the map slot
    assert ex[1] and ex[5] and not ex[2] and 2 < ex.sum() < 8
    assert np.array_equal(h['explored'].astype(bool), ex)
    assert np.array_equal(h['action'], np.where(ex, act, greedy[slots]))
    assert rng.step == 8
    _lib.check_faults()


# ---- 5. graph replay ---------------------------------------------------------------------------------------
def test_graph_replay_advances_the_rng_state(S, BIG):
    _lib, batch, context, synthetic = S
    from simaps import policy_output
    b, q, greedy = BIG
    s0 = 2 ** 32 - 2                                              # (the step crosses into its high word)
    rng = policy_output.DeviceExploration(99, b.device, step=s0)
    q_off = torch.arange(256, dtype=torch.int64, device=b.device) * 18432
    eps = torch.full((256,), 0.25, dtype=torch.float32, device=b.device)
    qf = q.reshape(-1)
    b.store_new_actions(q=qf, q_off=q_off, use_shortest_path_movement=False, max_points=2, exploration_eps=eps,
                        rng=policy_output.DeviceExploration(1, b.device))     # (first use outside the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        r = b.store_new_actions(q=qf, q_off=q_off, use_shortest_path_movement=False, max_points=2,
                                exploration_eps=eps, rng=rng)
    torch.cuda.synchronize()
    assert rng.step == s0                                         # capturing runs nothing
    for k in range(3):
        g.replay()
        torch.cuda.synchronize()
        ex, act = E.draws(99, s0 + k, 256, 0.25, 18432)
        assert np.array_equal(r.explored.cpu().numpy().astype(bool), ex), k
        assert np.array_equal(r.action.cpu().numpy(), np.where(ex, act, greedy)), k
    assert rng.step == s0 + 3
    _lib.check_faults()


# ---- 6. a bad eps is a contained descriptor error -----------------------------------------------------------
@pytest.mark.parametrize('bad', [float('nan'), 1.5, -0.1], ids=['nan', 'above_1', 'negative'])
def test_bad_eps_is_contained(S, bad):
    _lib, batch, context, synthetic = S
    from simaps import policy_output
    ctx = context.Context()
    try:
        scenes = [synthetic.make_scene(DIVIDER, 60 + e) for e in range(2)]
        g = torch.Generator().manual_seed(21)
        q = torch.randn(8, 2, 96, 96, generator=g).to(torch.bfloat16)

        def run(eps5):
            b = batch.StateBatch(scenes, context=ctx)
            eps = np.full(8, 0.5, dtype=np.float32)
            eps[5] = eps5
            rng = policy_output.DeviceExploration(3, b.device, step=11)
            return b, b.store_new_actions(q=q.to(b.device), max_points=16, exploration_eps=eps, rng=rng)

        want = run(0.5)[1].to_host()
        assert ctx.fault_info() == (0, None, None)
        ba, res = run(bad)
        got = res.to_host()                                       # (synchronises)
        assert got['count'][5] == 0 and got['explored'][5] == 0
        assert 0 < want['explored'].sum() < 8 and (want['count'] >= 2).all()
        for n in range(8):
            if n != 5:
                c = int(want['count'][n])
                assert got['count'][n] == c and got['action'][n] == want['action'][n]
                assert got['explored'][n] == want['explored'][n]
                assert got['xy'][n, :c].tobytes() == want['xy'][n, :c].tobytes()
                assert got['heading'][n, :c].tobytes() == want['heading'][n, :c].tobytes()
        assert ctx.fault_info() == (_lib.FAULT_DESCRIPTOR, 'action', 5)
        with pytest.raises(_lib.DeviceFault, match='in action, unit 5'):   # the context's next call, once
            ba.store_new_actions(q=q.to(ba.device), max_points=16)
        assert _lib.lib.simaps_fault_status(0) == 0               # not the default context
    finally:
        torch.cuda.synchronize()
        ctx.fault_status(clear=True)
        ctx.close()


# ---- 7. the Python surface ------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', sorted(DTYPES))
def test_store_new_actions_takes_16bit_q_in_its_three_forms(S, dt):
    _lib, batch, context, synthetic = S
    dtype = DTYPES[dt]
    b = batch.StateBatch([synthetic.make_scene(MIXED, 1)])
    g = torch.Generator().manual_seed(5)
    q = [torch.randn(2, k, 96, 96, generator=g).to(dtype).to(b.device) for k in (2, 1)]
    groups = [(q[0], [0, 1]), (q[1], [2, 3])]
    kw = dict(use_shortest_path_movement=False, max_points=2)
    want = b.store_new_actions(q=[(t.float(), p) for t, p in groups], **kw)          # the float32 call on q.float()
    got = b.store_new_actions(q=groups, **kw)                                         # the list form
    assert torch.equal(got.action, want.action) and got.explored is None
    flat = torch.cat([t.reshape(-1) for t in q])
    off = np.array([0, 18432, 36864, 36864 + 9216], dtype=np.int64)
    assert torch.equal(b.store_new_actions(q=flat, q_off=off, **kw).action, want.action)   # q and q_off
    lift = b.store_new_actions(q=q[0], slots=[0, 1], **kw)                             # [n, K, 96, 96]
    assert torch.equal(lift.action, want.action[:2])
    for k in ('source', 'target', 'xy', 'heading', 'count'):
        assert torch.equal(getattr(got, k), getattr(want, k)), k
    with pytest.raises(ValueError, match='different dtypes'):
        b.store_new_actions(q=[(q[0], [0, 1]), (q[1].float(), [2, 3])], **kw)
    with pytest.raises(ValueError):
        b.store_new_actions(q=flat.double(), q_off=off, **kw)
    with pytest.raises(ValueError, match='rng'):
        b.store_new_actions(q=groups, exploration_eps=0.5, **kw)
    _lib.check_faults()


def test_vector_env_explores_on_the_device_and_writes_back(S):
    _lib, batch, context, synthetic = S
    from simaps import policy_output, vector_env
    scenes = [synthetic.make_scene(DIVIDER, 920 + e) for e in range(2)]
    obs = vector_env.VectorEnvObservations(scenes, layout='chw')
    arr = _with_array_descriptors(S, obs.batch, scenes)
    P = _lib.MAX_PATH
    q = torch.zeros(4, 2, 96, 96, dtype=torch.bfloat16, device=obs.batch.device)
    outputs = [[(list(range(4)), q)], [(list(range(4)), q)]]
    action = [[[None, -1, None, -1]], [[None] * 4]]               # -1 or None: the device decides
    rng = policy_output.DeviceExploration(8, obs.batch.device, step=2)
    got = obs.store_new_action(action, outputs=outputs, max_points=P, write_back=True, exploration_eps=1.0, rng=rng)
    state1 = [t.clone() for e in obs.get_state(all_robots=True) for grp in e for t in grp]
    ex, act = E.draws(8, 2, 8, 1.0, 18432)
    assert ex.all() and rng.step == 3
    for e in range(2):
        for a in range(4):
            r, n = got[e][0][a], e * 4 + a
            assert r['explored'] is True
            assert r['action'] == tuple(int(v) for v in A.action_tuple(int(act[n]), 0))
            c = len(r['waypoint_positions'])
            arr['target'][n] = r['target_end_effector_position'][:2]
            arr['idle'][n] = False
            arr['waypoints'][n] = 0
            arr['waypoints'][n, :c] = [p[:2] for p in r['waypoint_positions']]
            arr['wp_count'][n] = c
            arr['wp_index'][n] = 1
    obs.update_arrays(**arr)                                      # the host route to the same descriptors
    state2 = [t for e in obs.get_state(all_robots=True) for grp in e for t in grp]
    for x, y in zip(state1, state2):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    # without exploration the dicts say so
    plain = obs.store_new_action([[[0, None, None, None]], [[None] * 4]], max_points=P)
    assert plain[0][0][0]['explored'] is False
    _lib.check_faults()
