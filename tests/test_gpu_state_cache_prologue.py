"""GPU: the cached get_state instance's prologue and late array fetch (csrc/simaps_spec_cached.hip).

The instance loads only what it uses of the record ahead of the verdict (the key on one wave, the window
words where a wave has window rows, the free bits on waves 0-3) and, on a hit, has waves 4-7 copy the
receptacle's array from the record into distance array 0 by LDS-DMA after the verdict, retired before
the distance phase.  None of that may change a value: every case renders 1 to 8 stacks of lifting_4-small_divider
(whose distance phase keeps its cell table in the tail of distance array 0, right behind the copied
array) and compares the whole stack, all five channels, with torch.equal against the uncached instance
of the same build (render(state_cache=False)); one scene also against the CPU oracle.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

FLAGSHIP = 'lifting_4-small_divider'
ROOM_H, ROOM_W = 44, 92
ARRAY_OFF = 2192                                # off_rec(44) + the array's 16-byte header (csrc/state_cache.h)
ARRAY_BYTES = (ROOM_H + 2) * ((ROOM_W + 2) | 1) * 4


@pytest.fixture(scope='module')
def S():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a GPU (run with -m gpu on an MI355X)')
    from simaps import _lib, batch, context, synthetic
    _lib.lib.simaps_fault_status(1)
    yield _lib, batch, context, synthetic
    _lib.lib.simaps_fault_status(1)


def _xy(b, row, col):
    c = b.cfg
    return (float((int(c.room_j0) + col + 0.5 - b.W / 2) / 96.0), float((b.H / 2 - (int(c.room_i0) + row + 0.5)) / 96.0), 0)


def _batch(S, seed, envs):
    _lib, batch, context, synthetic = S
    b = batch.StateBatch([synthetic.make_scene(FLAGSHIP, seed + e) for e in range(envs)])
    assert b.kernel_instance() == _lib.SPEC_S1 and b.room_class() == _lib.ROOM_SMALL
    assert (int(b.cfg.room_h), int(b.cfg.room_w)) == (ROOM_H, ROOM_W)
    assert _lib.lib.simaps_state_cache_bytes(b.cfg) >= ARRAY_OFF + ARRAY_BYTES
    return b


def _counters(b):
    hd = b.state_cache_headers()
    return hd['hits'].astype(int).tolist(), hd['misses'].astype(int).tolist()


def _render_pair(S, b, slots=None):
    got = b.render(slots=slots)
    ref = b.render(slots=slots, state_cache=False)
    torch.cuda.synchronize()
    S[0].check_faults()
    assert got.shape[1] == 5
    for c in range(5):
        assert torch.equal(got[:, c], ref[:, c]), 'channel %d differs from the uncached instance' % c
    assert not torch.isnan(got).any() and float(got.abs().max()) > 0
    return got


def _arrays(b):
    return b._state_cache[:, ARRAY_OFF:ARRAY_OFF + ARRAY_BYTES].cpu().numpy().copy()


def test_miss_hit_hit_one_env_against_the_oracle(S):
    b = _batch(S, seed=31, envs=1)
    outs = [_render_pair(S, b) for _ in range(3)]
    assert _counters(b) == ([2] * 4, [1] * 4)
    assert torch.equal(outs[1], outs[0]) and torch.equal(outs[2], outs[0])
    got = b.as_hwc(outs[2]).cpu().numpy()
    for n, (e, a) in enumerate(b.agents):
        ref = oracle.agent_state(b.scenes[e], a)
        assert got[n].shape == ref.shape and np.array_equal(got[n].view(np.uint32), ref.view(np.uint32)), \
            'a hit: stack %d differs from the oracle' % n


def test_miss_hit_hit_two_envs_each_slot_its_own_array(S):
    """Two envs with the receptacle in different places: a hit's array is the slot's own record's."""
    b = _batch(S, seed=33, envs=2)
    b.scenes[1]['receptacle_position'] = _xy(b, 6, 80)
    b.scenes[0]['receptacle_position'] = _xy(b, 38, 8)
    b.set_descriptors(b.scenes)
    outs = [_render_pair(S, b) for _ in range(3)]
    assert _counters(b) == ([2] * 8, [1] * 8)
    assert torch.equal(outs[1], outs[0]) and torch.equal(outs[2], outs[0])
    arr = _arrays(b)
    assert not np.array_equal(arr[0], arr[4])                             # the two envs' arrays do differ
    hd = b.state_cache_headers()
    assert len({(int(i), int(j)) for i, j in zip(hd['rec_i'], hd['rec_j'])}) == 2
    for k in (7, 0, 4):                                                   # and launches of one stack, all hits
        one = _render_pair(S, b, slots=[k])
        assert torch.equal(one[0], outs[0][k])
    mixed = _render_pair(S, b, slots=[6, 1, 3])
    assert all(torch.equal(mixed[n], outs[0][k]) for n, k in enumerate((6, 1, 3)))
    hits, misses = _counters(b)
    assert misses == [1] * 8 and hits == [3, 3, 2, 3, 3, 2, 3, 3]


def test_last_slot_beyond_the_cache(S):
    """cache_records one short of the launch's slots: the last slot computes everything, cold and warm,
    and neither reads nor writes the bytes where its record would have been."""
    _lib, batch, context, synthetic = S
    for envs in (1, 2):
        b = _batch(S, seed=35, envs=envs)
        ref = b.render(state_cache=False)
        nb = _lib.lib.simaps_state_cache_bytes(b.cfg)
        cache = torch.zeros((b.N, nb), dtype=torch.uint8, device=b.device)
        cache[b.N - 1] = 0xA5                                             # never a valid record, never touched
        for k in range(3):
            out = b.alloc_state()
            assert _lib.lib.simaps_get_state_cached(b.cfg, b.N, _lib.ptr(b.agents_d), _lib.ptr(b.envs_d), _lib.ptr(b.robots_d),
                                                    _lib.ptr(b.paths_d), _lib.ptr(b.occupancy), _lib.ptr(b.overhead),
                                                    _lib.ptr(out), 0, None, _lib.stream_handle(), _lib.ptr(cache), b.N - 1) == 0
            torch.cuda.synchronize()
            _lib.check_faults()
            assert torch.equal(out, ref)
        assert int(cache[b.N - 1].min()) == 0xA5 and int(cache[b.N - 1].max()) == 0xA5
        hd = cache[:, :80].cpu().numpy().copy().view(_lib.STATE_CACHE_HEADER_DTYPE).reshape(-1)
        assert hd['hits'].tolist()[:-1] == [2] * (b.N - 1) and hd['misses'].tolist()[:-1] == [1] * (b.N - 1)
    one = _batch(S, seed=36, envs=1)                                      # a launch of one stack with no record at all
    ref = one.render(slots=[2], state_cache=False)
    agents_d, n = one.subset_descriptor([2])
    cache = torch.full((2, _lib.lib.simaps_state_cache_bytes(one.cfg)), 0xA5, dtype=torch.uint8, device=one.device)
    for k in range(2):
        out = one.alloc_state(1)
        assert _lib.lib.simaps_get_state_cached(one.cfg, 1, _lib.ptr(agents_d), _lib.ptr(one.envs_d), _lib.ptr(one.robots_d),
                                                _lib.ptr(one.paths_d), _lib.ptr(one.occupancy), _lib.ptr(one.overhead),
                                                _lib.ptr(out), 0, None, _lib.stream_handle(), _lib.ptr(cache), 2) == 0
        torch.cuda.synchronize()
        _lib.check_faults()
        assert torch.equal(out, ref)
    assert int(cache.min()) == 0xA5 and int(cache.max()) == 0xA5


CORNERS = [(0, 0), (0, ROOM_W - 1), (ROOM_H - 1, 0), (ROOM_H - 1, ROOM_W - 1)]


@pytest.mark.parametrize('envs', [1, 2])
def test_tail_guard_robots_at_the_four_corners(S, envs):
    """The copied array ends 8 bytes before the distance phase's cell table (the array's tail): robots in
    the room's four corners sample the array's first and last rows and columns through that table, in a
    room without obstacles, so a copy that stops short of the array's end shows.  (A copy that ran over
    it into the table would not: the render track writes the table afterwards.  That bound is the
    kernel's static_assert.)  The second env turns its corners by one."""
    b = _batch(S, seed=37, envs=envs)
    i0, j0 = int(b.cfg.room_i0), int(b.cfg.room_j0)
    occ = []
    for e, scene in enumerate(b.scenes):
        for k, r in enumerate(scene['robots']):
            r['position'] = _xy(b, *CORNERS[(k + e) % 4])
            r['waypoint_positions'] = [r['position']] + list(r['waypoint_positions'][1:])
        scene['receptacle_position'] = _xy(b, ROOM_H - 1, ROOM_W // 2 + e)
        o = np.array(scene['occupancy'][0], dtype=np.uint8)
        o[i0:i0 + ROOM_H, j0:j0 + ROOM_W] = 0
        occ += [o] * 4
    b.set_descriptors(b.scenes)
    b.set_maps(occupancy=np.stack(occ))
    cold = _render_pair(S, b)
    for k in range(2):
        assert torch.equal(_render_pair(S, b), cold)
    assert _counters(b) == ([2] * b.N, [1] * b.N)
    for k in range(b.N):                                                  # and one stack at a time
        assert torch.equal(_render_pair(S, b, slots=[k])[0], cold[k])


def test_descriptor_clamp_posts_the_same_fault_as_the_uncached_path(S):
    """An agent's robot index past num_robots, with the record's loads trimmed around the clamp: the same
    fault word and `where`, and the same stacks, from simaps_get_state and from a cold and two warm
    simaps_get_state_cached; also as a launch of that one agent."""
    _lib, batch, context, synthetic = S
    b = _batch(S, seed=39, envs=2)
    robots, envs, ag, paths = batch.pack_descriptors(b.scenes, b.agents)
    robots = np.concatenate([robots, np.repeat(robots[:1], 8)])
    paths = np.concatenate([paths, np.repeat(paths[:1], 40, 0)])
    ag['robot'][5] = 6                                                    # 8 agents, only agent 5 is bad
    R, E, A = (batch._to_dev(x, b.device) for x in (robots, envs, ag))
    A1 = batch._to_dev(ag[5:6].copy(), b.device)
    P = torch.from_numpy(paths).to(b.device)
    cache = torch.zeros((b.N, _lib.lib.simaps_state_cache_bytes(b.cfg)), dtype=torch.uint8, device=b.device)
    ctx = context.Context()
    try:
        for agents, n, unit in ((A, b.N, 5), (A1, 1, 0)):
            got = []
            for entry in ('get_state', 'get_state_cached', 'get_state_cached', 'get_state_cached'):
                out = b.alloc_state(n)
                extra = () if entry == 'get_state' else (_lib.ptr(cache), b.N)
                rc = _lib.call(ctx, entry, b.cfg, n, _lib.ptr(agents), _lib.ptr(E), _lib.ptr(R), _lib.ptr(P),
                               _lib.ptr(b.occupancy), _lib.ptr(b.overhead), _lib.ptr(out), 0, None, _lib.stream_handle(), *extra)
                assert rc == 0
                torch.cuda.synchronize()
                k, u = ctypes.c_int(-2), ctypes.c_int(-2)
                bits = _lib.lib.simaps_ctx_fault_info(ctx.handle, 0, ctypes.byref(k), ctypes.byref(u))
                got.append((bits, k.value, u.value, ctx.fault_info(clear=True), out))
            for bits, k, u, info, out in got:
                assert (bits, k, u) == (_lib.FAULT_DESCRIPTOR, 1, unit)          # SIMAPS_K_GET_STATE
                assert info == (_lib.FAULT_DESCRIPTOR, 'get_state', unit)
                assert torch.equal(out, got[0][4])
        hd = cache[:, :80].cpu().numpy().copy().view(_lib.STATE_CACHE_HEADER_DTYPE).reshape(-1)
        assert hd['misses'].tolist() == [1] * 8 and hd['hits'].tolist() == [2, 2, 2, 2, 2, 5, 2, 2]
    finally:
        torch.cuda.synchronize()
        ctx.fault_status(clear=True)
        ctx.close()


def test_late_array_the_distance_phase_waits_for_the_data(S):
    """The diagnostic library (SIMAPS_DIAG_ARRAY_LATE) has a hit's waves 4-7 issue the array's fetch only
    when they arrive at the workgroup barrier ahead of the distance phase, with none of their own work
    left to hide it: their wait for it and that barrier are all that stands between the fetch and the
    distance phase's reads, which follow at once.  The same stacks, cold and warm, launches of 8 and of
    1, no timeout flag.  (Run once with the wait taken out of that library, the warm launches gave other
    stacks: DESIGN.md.)"""
    _lib, batch, context, synthetic = S
    lib = os.path.join(os.path.dirname(_lib.__file__), 'libsimaps_diagring.so')
    if not os.path.exists(lib):
        pytest.fail('build the diagnostic library first: make -C spatial-intention-maps_amd/csrc diag')
    L = _lib._load(lib)
    assert L.simaps_fault_status(1) == 0
    b = _batch(S, seed=41, envs=2)
    b.scenes[1]['receptacle_position'] = _xy(b, 6, 80)
    b.set_descriptors(b.scenes)
    ref = b.render(state_cache=False)
    cache = torch.zeros((b.N, L.simaps_state_cache_bytes(b.cfg)), dtype=torch.uint8, device=b.device)

    # (a workgroup's LDS is not cleared between launches: without this render of 256 other stacks, one per
    # CU, a launch could find its own earlier copy of the array still in distance array 0)
    other = _batch(S, seed=141, envs=64)

    def launch(agents_d, n):
        other.render(state_cache=False)
        out = b.alloc_state(n)
        assert L.simaps_get_state_cached(b.cfg, n, _lib.ptr(agents_d), _lib.ptr(b.envs_d), _lib.ptr(b.robots_d),
                                         _lib.ptr(b.paths_d), _lib.ptr(b.occupancy), _lib.ptr(b.overhead), _lib.ptr(out), 0,
                                         None, _lib.stream_handle(), _lib.ptr(cache), b.N) == 0
        torch.cuda.synchronize()
        assert L.simaps_fault_status(0) == 0
        return out
    for k in range(3):
        assert torch.equal(launch(b.agents_d, b.N), ref)
    for k in (6, 2):
        agents_d, n = b.subset_descriptor([k])
        assert torch.equal(launch(agents_d, n)[0], ref[k])
    hd = cache[:, :80].cpu().numpy().copy().view(_lib.STATE_CACHE_HEADER_DTYPE).reshape(-1)
    assert hd['misses'].tolist() == [1] * 8 and hd['hits'].tolist() == [2, 2, 3, 2, 2, 2, 3, 2]
