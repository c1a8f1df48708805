"""GPU: the state cache (include/simaps_state_cache.h) over whole episodes and over every bit of the
compared window, against the CPU oracle and the host model of tests/state_cache_model.py.

tests/test_gpu_state_cache.py checks single transitions against the same build; here a record outlives
many changes (tests/state_cache_episodes.py scripts them: new poses, blocks, re-uploads, byte values
other than 1, pixels just outside the compared block, the receptacle inside and out of its pixel, a
robot class, env resets, subset / permuted / repeated launches, map A -> B -> A with and without a
render at B, device-side ingest), a captured graph replays across hits and misses, two streams share
the cache, and each of the 58 x 144 compared pixels is toggled once on its own.  Every stack is
compared bit for bit; the records' counters must equal the model's.
"""
import numpy as np
import pytest
import torch

import oracle
import state_cache_episodes as EP
import state_cache_model as M

pytestmark = pytest.mark.gpu

FLAGSHIP = EP.FLAGSHIP


@pytest.fixture(scope='module')
def S():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a GPU (run with -m gpu on an MI355X)')
    from simaps import _lib, batch, synthetic
    _lib.lib.simaps_fault_status(1)
    yield _lib, batch, synthetic
    _lib.lib.simaps_fault_status(1)


def _u32(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _counters(b):
    hd = b.state_cache_headers()
    return hd['hits'].astype(int).tolist(), hd['misses'].astype(int).tolist()


def _against_oracle(b, out, slots, what, last_op=None):
    """Stack n of `out` (map slot slots[n]) equals the oracle's bit for bit."""
    got = b.as_hwc(out).cpu().numpy()
    for n, s in enumerate(slots):
        e, a = b.agents[s]
        ref = oracle.agent_state(b.scenes[e], a)
        if got[n].shape != ref.shape or not np.array_equal(_u32(got[n]), _u32(ref)):
            bad = np.argwhere(_u32(got[n]) != _u32(ref))
            pytest.fail('%s: slot %d (stack %d of the launch) differs from the oracle in %d values, first at (row, col, channel) '
                        '%s: %r != %r%s' % (what, s, n, len(bad), tuple(int(x) for x in bad[0]), float(got[n][tuple(bad[0])]),
                                            float(ref[tuple(bad[0])]),
                                            '' if last_op is None else '; last operation on the slot: ' + last_op[s]))
    return len(slots)


def _run(b, batch, ep, cmd):
    if cmd[0] == 'set_descriptors':
        b.set_descriptors(ep.scenes)
    elif cmd[0] == 'set_descriptor_arrays':
        b.set_descriptor_arrays(**batch.descriptor_arrays(ep.scenes))
    elif cmd[0] == 'set_maps':
        b.set_maps(occupancy=cmd[2], overhead=cmd[3], slots=cmd[1])
    elif cmd[0] == 'ingest':
        b.ingest(cmd[2], cmd[3], slots=cmd[1])
    else:
        raise AssertionError(cmd[0])


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_episode_against_the_oracle_and_the_model(S, seed):
    _lib, batch, synthetic = S
    ep = EP.Episode(seed)
    b = batch.StateBatch(ep.scenes)
    assert b.kernel_instance() == _lib.SPEC_S1 and b.room_class() == _lib.ROOM_SMALL and M.uses_cache(b.cfg)
    stacks = 0
    for st in ep.steps():
        for cmd in st.cmds:
            _run(b, batch, ep, cmd)
        for slots in st.launches:
            what = 'seed %d step %d (%s) launch of slots %s' % (seed, st.k, st.unit, slots)
            out = b.render(slots=slots)
            torch.cuda.synchronize()
            _lib.check_faults()
            outcome = ep.launch(st, slots)
            stacks += _against_oracle(b, out, slots, what, ep.last_op)
            hits, misses = _counters(b)
            for s in range(ep.N):
                assert (hits[s], misses[s]) == (ep.model.hits[s], ep.model.misses[s]), \
                    '%s: slot %d has (hits, misses) (%d, %d), the model (%d, %d), this launch %s; last operation on the slot: %s' % (
                        what, s, hits[s], misses[s], ep.model.hits[s], ep.model.misses[s],
                        dict(zip(slots, outcome)).get(s, 'not rendered'), ep.last_op[s])
    totals = ep.finish()
    hd = b.state_cache_headers()
    for s in range(ep.N):  # the records' keys are the model's
        assert tuple(int(hd[f][s]) for f in M.KEY_FIELDS) == ep.model.records[s][0], s
    print('episode totals', dict(totals, oracle_stacks=stacks))


def test_graph_replay_across_hits_and_misses(S):
    """One captured render(out=fixed) replayed four times: unchanged (hit), a pixel written in place
    (miss), unchanged (hit), the pixel restored (miss)."""
    _lib, batch, synthetic = S
    scenes = [synthetic.make_scene(FLAGSHIP, 31)]
    b = batch.StateBatch(scenes)
    c = M.config_of(scenes[0])
    model = M.Model(b.N, lambda s: (M.key(c, scenes[0], s), M.window_bits(scenes[0]['occupancy'][s], c)))
    fixed = b.alloc_state()
    b.render(out=fixed)                                                 # allocates the cache: the cold miss
    model.render()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        b.render(out=fixed)
    slot, (i, j) = 2, (c.room_i0 + 20, c.room_j0 + 31)
    old = int(scenes[0]['occupancy'][slot][i, j])
    for k, (value, want) in enumerate([(None, 'hit'), (0 if old else 1, 'miss'), (None, 'hit'), (old, 'miss')]):
        if value is not None:
            b.occupancy[slot, i, j] = value
            scenes[0]['occupancy'][slot][i, j] = value
        fixed.fill_(float('nan'))
        g.replay()
        torch.cuda.synchronize()
        _lib.check_faults()
        got = model.render()
        assert got[slot] == want and [o for n, o in enumerate(got) if n != slot] == ['hit'] * 3
        _against_oracle(b, fixed, range(b.N), 'replay %d' % k)
        assert _counters(b) == (model.hits, model.misses), 'replay %d' % k
    assert _counters(b) == ([4, 4, 2, 4], [1, 1, 3, 1])


def test_two_streams_share_the_cache(S):
    """A cold render on stream s1, a second on s2 with nothing between them but the batch's own
    ordering of the cache's users (a hit on the records the first is still writing), then the map
    written behind the second render and a third render on s1 after the caller's event (a miss)."""
    _lib, batch, synthetic = S
    scenes = [synthetic.make_scene(FLAGSHIP, 33), synthetic.make_scene(FLAGSHIP, 34)]
    b = batch.StateBatch(scenes)
    c = M.config_of(scenes[0])
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    first = b.render(stream=s1)
    second = b.render(stream=s2)
    slot, (i, j) = 5, (c.room_i0 - 7, M.window_a0(c))                  # the compared block's first pixel
    e, a = b.agents[slot]
    value = 0 if scenes[e]['occupancy'][a][i, j] else 0x40
    with torch.cuda.stream(s2):
        b.occupancy[slot, i, j] = value                                  # behind the second render, in s2's order
    ev = torch.cuda.Event()
    ev.record(s2)
    s1.wait_event(ev)
    third = b.render(stream=s1)
    torch.cuda.synchronize()
    _lib.check_faults()
    assert torch.equal(first.view(torch.int32), second.view(torch.int32))
    _against_oracle(b, first, range(b.N), 'the render on s1')
    _against_oracle(b, second, range(b.N), 'the render on s2')
    scenes[e]['occupancy'][a][i, j] = value
    _against_oracle(b, third, range(b.N), 'the render on s1 after the map write')
    assert _counters(b) == ([2 - (s == slot) for s in range(b.N)], [1 + (s == slot) for s in range(b.N)])


# ---- every bit of the compared window
WIN_ROWS, WIN_COLS = 58, M.WIN_BYTES
RUN = 261                                                               # 58 * 144 = 32 slots x 261 pixels, row-major


def _pixel_name(p):
    r, col = divmod(p, WIN_COLS)
    return 'window row %d, byte column %d, word %d, bit %d' % (r, col, col // 32, col % 32)


def test_every_bit_of_the_compared_window(S):
    """32 slots; slot k toggles pixels 261 k .. 261 k + 260 of the compared block one per step and never
    back, so each step's map differs from the slot's record in exactly that pixel: every step is a
    miss in every slot, and the stacks equal the uncached instance's; every 29 steps a second render
    hits everywhere and the stacks are compared with the oracle."""
    _lib, batch, synthetic = S
    scenes = [synthetic.make_scene(FLAGSHIP, 40 + e) for e in range(8)]
    b = batch.StateBatch(scenes)
    c, N = b.cfg, b.N
    assert N == 32 and N * RUN == WIN_ROWS * WIN_COLS == 8352 and M.uses_cache(c)
    assert (c.room_h + 2 * M.PAD, M.window_a0(c), M.window_a0(c) + WIN_COLS <= b.W) == (WIN_ROWS, 60, True)
    host = [scenes[e]['occupancy'][a] for e, a in b.agents]             # (views: the oracle reads the toggles)
    idx = np.zeros((RUN, N), dtype=np.int64)
    val = np.zeros((RUN, N), dtype=np.uint8)
    toggled = np.zeros(WIN_ROWS * WIN_COLS, dtype=np.int64)
    for k in range(RUN):
        for s in range(N):
            p = s * RUN + k
            i, j = M.window_pixel(c, *divmod(p, WIN_COLS))
            idx[k, s] = (s * b.H + i) * b.W + j
            val[k, s] = 0 if host[s][i, j] else 1
    idx_d, val_d = torch.from_numpy(idx).to(b.device), torch.from_numpy(val).to(b.device)
    flat = b.occupancy.view(-1)
    b.render()
    torch.cuda.synchronize()
    assert _counters(b) == ([0] * N, [1] * N)
    hit_checks = oracle_stacks = 0
    for k in range(RUN):
        flat[idx_d[k]] = val_d[k]                                       # one indexed write: all 32 slots' pixels
        for s in range(N):
            host[s].reshape(-1)[idx[k, s] - s * b.H * b.W] = val[k, s]
            toggled[s * RUN + k] += 1
        got = b.render()
        ref = b.render(state_cache=False)
        same = (got.view(torch.int32) == ref.view(torch.int32)).flatten(1).all(1).cpu().numpy()
        hits, misses = _counters(b)
        _lib.check_faults()
        for s in range(N):
            where = 'step %d slot %d, toggled pixel %d (%s)' % (k, s, s * RUN + k, _pixel_name(s * RUN + k))
            assert (hits[s], misses[s]) == (hit_checks, k + 2), \
                '%s: (hits, misses) (%d, %d), expected (%d, %d): the compare did not see the pixel' % (
                    where, hits[s], misses[s], hit_checks, k + 2)
            assert same[s], '%s: the cached render differs from the uncached instance' % where
        if k % 29 == 28:
            again = b.render()
            torch.cuda.synchronize()
            hit_checks += 1
            assert _counters(b) == ([hit_checks] * N, [k + 2] * N), 'step %d: an unchanged map did not hit' % k
            assert torch.equal(again.view(torch.int32), got.view(torch.int32))
            oracle_stacks += _against_oracle(b, again, range(N), 'step %d' % k)
    assert (toggled == 1).all() and int(toggled.sum()) == 8352          # no pixel skipped, none twice
    assert np.array_equal(b.occupancy.cpu().numpy(), np.stack(host))
    assert hit_checks == 9 and oracle_stacks == 9 * N
    print('window bits toggled %d, hit checks %d x %d slots, oracle stacks %d' % (int(toggled.sum()), hit_checks, N, oracle_stacks))
