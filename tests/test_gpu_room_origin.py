"""GPU: get_state with the room rectangle moved inside the map.  room_i0 / room_j0 are run-time
values of every compile-time instance (include/simaps_spec_room.h); every other GPU test uses the
centred origin (70, 70), where the occupancy window's alignment is sub = (room_j0 - 7) & 3 = 3.

Here: the other three alignments, the last origin on the 4-byte window loads (room_j0 = 98, the
load that ends on the row's last byte) and the first ones on the byte fallback (99 and 6, which also
go without the state cache), and window rows and columns outside the map.  Per origin one env, four
stacks, each path bit for bit against the oracle with the same rectangle (scene['room_rect']): the
cached render cold and warm, the uncached instance, the generic kernel and its cspace, a float32
store, and the bfloat16 render.

Robots and receptacle stay where the synthetic scene put them; where the rectangle no longer holds
them, their sources are snapped to the nearest free cell (the oracle's EDT, the kernel's snap_wave).
"""
import numpy as np
import pytest
import torch

import oracle
import state_cache_model as M

pytestmark = pytest.mark.gpu

FLAGSHIP = 'lifting_4-small_divider'
H, W, RH, RW = M.SMALL
ORIGINS = [(70, 68), (70, 69), (70, 71), (70, 72), (68, 70), (72, 70),      # sub = 1, 2, 0, 1; rows moved
           (70, 98), (70, 99), (70, 7), (70, 6),                            # the 4-byte loads' last and first origins
           (0, 0), (140, 140), (3, 70), (137, 70)]                          # window rows / columns outside the map


@pytest.fixture(scope='module')
def S():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a GPU (run with -m gpu on an MI355X)')
    from simaps import _lib, batch, synthetic
    _lib.lib.simaps_fault_status(1)
    yield _lib, batch, synthetic
    _lib.lib.simaps_fault_status(1)


def draw_occupancy(i0, j0, agent):
    """An occupancy map for the rectangle at (i0, j0): the rectangle free except a divider and a few
    blocks (some with byte values other than 1); a block across each side of the rectangle and one
    wholly outside each side, all within the 7-pixel margin; the window's corner pixels; and noise
    everywhere the window does not reach (alignment padding included), which must not matter."""
    rs = np.random.RandomState(1000 * i0 + 10 * j0 + agent)
    occ = np.zeros((H, W), dtype=np.uint8)
    noise = rs.random_sample((H, W)) < 0.3
    noise[max(i0 - 7, 0):i0 + RH + 7, max(j0 - 7, 0):j0 + RW + 7] = False
    occ[noise] = rs.choice([1, 0x02, 0x10, 0x80, 0xff], int(noise.sum()))

    def put(r0, r1, c0, c1, v=1):  # rows r0..r1-1, columns c0..c1-1 relative to the rectangle, clipped to the map
        occ[max(i0 + r0, 0):max(min(i0 + r1, H), 0), max(j0 + c0, 0):max(min(j0 + c1, W), 0)] = v

    put(8, 36, 45, 47)                                                      # the divider
    put(-3, 2, 20, 25), put(RH - 2, RH + 3, 60, 65), put(15, 20, -3, 2), put(25, 30, RW - 2, RW + 3, 0x04)
    put(-7, -4, 50, 53), put(RH + 4, RH + 7, 10, 13, 0x20), put(30, 33, -7, -4, 0x40), put(5, 8, RW + 4, RW + 7)
    put(-7, -6, -7, -6, 0x80), put(RH + 6, RH + 7, RW + 6, RW + 7, 0x80), put(-7, -6, RW + 6, RW + 7), put(RH + 6, RH + 7, -7, -6)
    put(5, 8, 70, 74, 0x10), put(36, 40, 12, 15, 0x80)
    r, c = rs.randint(0, RH - 4), rs.randint(0, RW - 4)                      # one block of the agent's own
    put(r, r + 3, c, c + 3, 0x08)
    return occ


def _u32(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _same(got, ref, what):
    if got.shape != ref.shape or not np.array_equal(_u32(got), _u32(ref)):
        bad = np.argwhere(_u32(got) != _u32(ref))
        pytest.fail('%s differs from the oracle in %d values, first at (row, col, channel) %s: %r != %r'
                    % (what, len(bad), tuple(int(x) for x in bad[0]), float(got[tuple(bad[0])]), float(ref[tuple(bad[0])])))


@pytest.mark.parametrize('i0, j0', ORIGINS, ids=['%d_%d' % o for o in ORIGINS])
def test_room_origin(S, i0, j0):
    _lib, batch, synthetic = S
    scene = synthetic.make_scene(FLAGSHIP, 17)
    scene['room_rect'] = (i0, j0, RH, RW)
    scene['occupancy'] = np.stack([draw_occupancy(i0, j0, a) for a in range(4)])
    b = batch.StateBatch([scene])
    b.cfg.room_i0, b.cfg.room_j0 = i0, j0
    assert (b.H, b.W, b.cfg.room_h, b.cfg.room_w) == (H, W, RH, RW) and 0 <= i0 <= H - RH and 0 <= j0 <= W - RW
    for dt, into in ((None, False), (torch.bfloat16, False), (torch.float32, True)):
        assert b.kernel_instance(dtype=dt, into=into) == _lib.SPEC_S1 and b.room_class(dtype=dt, into=into) == _lib.ROOM_SMALL
    assert b.kernel_instance(debug=True) == _lib.SPEC_GENERIC
    agents = [oracle.AgentOracle(scene, a) for a in range(4)]
    refs = [ag.get_state() for ag in agents]
    where = 'origin (%d, %d), sub %d: ' % (i0, j0, (j0 - 7) & 3)

    def check(out, what, cast=None):
        torch.cuda.synchronize()
        _lib.check_faults()
        got = b.as_hwc(out)
        for a in range(4):
            if cast is None:
                _same(got[a].cpu().numpy(), refs[a], where + what + ', agent %d' % a)
            else:
                want = torch.from_numpy(refs[a]).to(cast)
                assert torch.equal(got[a].cpu().view(torch.int16), want.view(torch.int16)), where + what + ', agent %d' % a

    cached = M.uses_cache(b.cfg)
    assert cached == (j0 >= 7 and ((j0 - 7) & ~3) + 144 <= W)
    for k, what in enumerate(('render() cold', 'render() warm')):
        check(b.render(), what)
        hd = b.state_cache_headers()
        if cached:
            assert (hd['hits'].tolist(), hd['misses'].tolist()) == ([k] * 4, [1] * 4), where + what
            assert (hd['room_i0'].tolist(), hd['room_j0'].tolist()) == ([i0] * 4, [j0] * 4)
        else:  # the records are allocated and passed, and the library leaves them alone
            assert hd is not None and not b._state_cache.any(), where + 'a call outside the cache rule wrote a record'
    check(b.render(state_cache=False), 'render(state_cache=False)')
    dbg = b.alloc_debug()
    check(b.render(debug=dbg), 'the generic kernel')
    cs = dbg['cspace'].cpu().numpy()
    for a in range(4):
        assert np.array_equal(cs[a], agents[a].cspace[i0:i0 + RH, j0:j0 + RW]), where + 'cspace of agent %d' % a
    store = b.alloc_store(6)
    store.fill_(float('nan'))
    dest = [3, 0, 5, 1]
    b.render_into(store, dest)
    check(store[dest], 'render_into a float32 store')
    assert torch.isnan(store[[2, 4]]).all()
    check(b.render(dtype=torch.bfloat16), 'render(dtype=bfloat16)', cast=torch.bfloat16)
