"""GPU: the sweep track's serial-overhead levers of the compile-time instances (csrc/simaps_spec.hip:
GS_SPEC_ROUND_WORD, GS_SPEC_FLAT_MARKS, GS_SPEC_EARLY_OCC, GS_SPEC_EARLY_ZERO)
against the generic kernel of the same build, which keeps the barrier + change-flag rounds, the lane-0
marks, the occupancy loads behind the entry barrier and the scratch
zeroing at the raster start.

A render() without debug buffers takes an instance, render(debug=...) the generic kernel; the two
states must be torch.equal.  Every case renders at most 8 stacks.  The round counts a case is there
for cannot be read through an instance (a debug pointer selects the generic kernel), so they are
asserted from the generic kernel's status word: a condition on the inputs.

Hand-made rooms are drawn into the occupancy maps with set_maps, in room-rect pixels; with a
configuration-space radius of 5 a one-pixel wall blocks 11 columns / rows, and an 11-pixel gap in
it leaves a one-pixel door.  A source is not src_ok only where its room has no free cell at all, and
then so is the stack's other source (they share the configuration space): such a stack is rendered
in the same launch as normal ones; a source on a blocked pixel (snapped) shares its workgroup with a
normal one.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FLAGSHIP = 'lifting_4-small_divider'
S2_NAME = 'rescue_4-small_empty'
LARGE = 'lifting_2_throwing_2-large_empty'     # 92 x 92 room, robot types with cspace radius 5 and 6
RMAX = 7                                       # the occupancy window's margin around the room rect (csrc)


@pytest.fixture(scope='module')
def S():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a GPU (run with -m gpu on an MI355X)')
    from simaps import _lib, batch, context, synthetic
    _lib.lib.simaps_fault_status(1)
    yield _lib, batch, context, synthetic
    _lib.lib.simaps_fault_status(1)


def _both(S, b, want):
    """(instance render, generic render, the generic kernel's status words) of batch b."""
    _lib = S[0]
    assert b.N <= 8
    assert b.kernel_instance() == want and b.kernel_instance(debug=True) == _lib.SPEC_GENERIC
    dbg = b.alloc_debug()
    spec = b.render()
    gen = b.render(debug=dbg)
    torch.cuda.synchronize()
    _lib.check_faults()
    st = dbg['status'].cpu().numpy()
    assert ((st & 14) == 0).all()                                        # no round cap, timeout or clamp
    return spec, gen, st, dbg


def _rect(b):
    c = b.cfg
    return int(c.room_i0), int(c.room_j0), int(c.room_h), int(c.room_w)


def _place(b, scene, cells):
    """Robot k of the scene onto room-rect cell cells[k] (row, column): the centre of that pixel."""
    i0, j0, h, w = _rect(b)
    for r, (row, col) in zip(scene['robots'], cells):
        x = (j0 + col + 0.5 - b.W / 2) / 96.0
        y = (b.H / 2 - (i0 + row + 0.5)) / 96.0
        r['position'] = (float(x), float(y), 0)
        r['waypoint_positions'] = [r['position']] + list(r['waypoint_positions'][1:])


def _draw(b, scene, walls, fill=False):
    """The scene's occupancy with the room interior cleared (or filled) and `walls` drawn, each
    (row0, row1, col0, col1) inclusive in room-rect pixels; one map for every agent of the scene."""
    i0, j0, h, w = _rect(b)
    occ = np.array(scene['occupancy'][0], dtype=np.uint8)
    occ[i0:i0 + h, j0:j0 + w] = 1 if fill else 0
    for r0, r1, c0, c1 in walls:
        occ[i0 + r0:i0 + r1 + 1, j0 + c0:j0 + c1 + 1] = 1
    return occ


def _serpentine(h, w, first=14, step=16, gap=14):
    """Vertical one-pixel walls every `step` columns, open for `gap` rows at alternating ends."""
    walls = []
    for k, c in enumerate(range(first, w - 8, step)):
        walls.append((0, h - 1 - gap, c, c) if k % 2 == 0 else (gap, h - 1, c, c))
    return walls


def _box(r0, r1, c0, c1):
    return [(r0, r0, c0, c1), (r1, r1, c0, c1), (r0, r1, c0, c0), (r0, r1, c1, c1)]


def _batch(S, name, seeds, cells, maps):
    """StateBatch of make_scene(name, seed) per seed, robots placed on `cells`, env e's maps drawn by
    maps[e](batch, scene)."""
    _lib, batch, context, synthetic = S
    scenes = [synthetic.make_scene(name, s) for s in seeds]
    b = batch.StateBatch(scenes)
    for sc in scenes:
        _place(b, sc, cells)
    b.set_descriptors(scenes)
    occ = np.concatenate([np.repeat(m(b, sc)[None], len(sc['robots']), 0) for m, sc in zip(maps, scenes)])
    b.set_maps(occupancy=occ)
    return b


SMALL_CELLS = [(38, 5), (38, 7), (36, 6), (34, 6)]      # the first serpentine corridor's open end


def _rounds_case(S, name, want):
    """Env 0: a serpentine room (the robots at one end, so the far cells need many rounds; in S1 the
    receptacle source at the other end has its own count).  Env 1: a room without any free cell
    (both sources not src_ok: one round)."""
    b = _batch(S, name, (3, 4), SMALL_CELLS,
               [lambda b, sc: _draw(b, sc, _serpentine(*_rect(b)[2:])), lambda b, sc: _draw(b, sc, [], fill=True)])
    spec, gen, st, dbg = _both(S, b, want)
    rounds = st >> 8
    print('rounds per stack:', rounds.tolist(), 'status bits:', (st & 15).tolist())
    assert rounds[:4].max() >= 7                    # the three round words are each reused twice
    assert (rounds[4:] <= 2).all() and (st[4:] & 1).all()               # and a stack that ends at once
    assert torch.equal(spec, gen)
    return b, dbg


def test_round_words_rotate_through_seven_rounds_beside_a_one_round_stack(S):
    """Within stack 0, two sources with different round counts.  The status word holds the maximum over
    the two sources only, so each source's own count is taken from the generic kernel on the same
    room with both sources on one pixel: the receptacle moved onto robot 0's cell, then robot 0 moved
    onto the receptacle's cell.  The two counts must differ and the larger one is the stack's."""
    _lib, batch, context, synthetic = S
    b, dbg = _rounds_case(S, FLAGSHIP, 1)
    both = int(dbg['status'][0]) >> 8
    src = dbg['sources'].cpu().numpy()
    i0, j0, h, w = _rect(b)
    assert (src[:4, 0, 3] - j0 > w - 16).all() and (src[:4, 1, 3] - j0 < 14).all()
    rec_cell = (int(src[0, 0, 2]) - i0, int(src[0, 0, 3]) - j0)
    own = []
    for cell in (SMALL_CELLS[0], rec_cell):                             # the robot's count, the receptacle's
        scene = synthetic.make_scene(FLAGSHIP, 3)
        b1 = batch.StateBatch([scene])
        _place(b1, scene, [cell] * 4)
        scene['receptacle_position'] = _xy(b1, *cell)
        b1.set_descriptors([scene])
        b1.set_maps(occupancy=np.repeat(_draw(b1, scene, _serpentine(h, w))[None], 4, 0))
        spec, gen, st, d1 = _both(S, b1, 1)
        s1 = d1['sources'].cpu().numpy()
        assert (s1[0, 0, 2:] == s1[0, 1, 2:]).all() and (s1[0, 0, 2:] == s1[0, 0, :2]).all()   # one free pixel
        assert torch.equal(spec, gen)
        own.append(int(st[0]) >> 8)
    print('rounds of stack 0: both sources', both, 'robot source alone', own[0], 'receptacle source alone', own[1])
    assert own[0] != own[1] and max(own) == both


def test_round_words_one_source_instance(S):
    _rounds_case(S, S2_NAME, 2)


BOTH = [(FLAGSHIP, 1), (S2_NAME, 2)]     # S1 (two sources, 8 sweep waves), S2 (one source, 4 sweep waves)


@pytest.mark.parametrize('name, want', BOTH)
def test_snapped_source_beside_a_normal_source(S, name, want):
    """Robots 0 and 1 on wall pixels (sources on blocked pixels: the snap slow path), robots 2 and 3
    free; the receptacle source of each S1 stack is a normal one (S2 has the robot source only: its
    debug record of the receptacle source is -1 throughout, so never "snapped")."""
    cells = [(10, 14), (43, 30), (38, 5), (38, 40)]
    b = _batch(S, name, (5,), cells, [lambda b, sc: _draw(b, sc, _serpentine(*_rect(b)[2:]))])
    spec, gen, st, dbg = _both(S, b, want)
    src = dbg['sources'].cpu().numpy()
    snapped = (src[:, :, :2] != src[:, :, 2:]).any(2)
    print('snapped sources:', snapped.tolist(), 'rounds:', (st >> 8).tolist())
    assert snapped[0, 1] and snapped[1, 1] and not snapped[:, 0].any() and not snapped[2:, 1].any()
    assert ((src[:, 0] >= 0).all() if want == 1 else (src[:, 0] == -1).all()) and (src[:, 1] >= 0).all()
    assert torch.equal(spec, gen)


@pytest.mark.parametrize('name, want', BOTH)
@pytest.mark.parametrize('door', ['vertical_wall', 'horizontal_wall'])
def test_marks_with_a_one_pixel_door_and_an_enclosed_pocket(S, door, name, want):
    """A wall across the room with an 11-pixel gap (a one-pixel door at radius 5) and a closed box
    (unreachable free cells inside).  Through the door the last improving rounds lower a few lines of
    a few lanes only: of the 2-cell row sweeps with the door in a vertical wall, of the 1-cell column
    sweeps with the door in a horizontal one (44 rows: one cell per lane)."""
    if door == 'vertical_wall':
        walls = [(0, 15, 46, 46), (27, 43, 46, 46)] + _box(10, 32, 60, 80)
        cells = [(22, 10), (8, 20), (36, 30), (22, 36)]
    else:
        walls = [(22, 22, 0, 39), (22, 22, 51, 91)] + _box(24, 43, 60, 80)
        cells = [(34, 10), (34, 20), (36, 30), (32, 52)]
    b = _batch(S, name, (6,), cells, [lambda b, sc: _draw(b, sc, walls)])
    spec, gen, st, dbg = _both(S, b, want)
    cs = dbg['cspace'].cpu().numpy()[0].astype(bool)
    d = dbg['dist'].cpu().numpy()[0]
    print('rounds:', (st >> 8).tolist(), 'free cells:', int(cs.sum()), 'door:', door)
    if door == 'vertical_wall':
        assert cs[:, 46].sum() == 1 and cs[21, 46]                       # the one-pixel door
    else:
        assert cs[22, :].sum() == 1 and cs[22, 45]
    pocket = cs[14:29, 66:75] if door == 'vertical_wall' else cs[30:38, 66:75]
    assert pocket.any()                                                  # free cells inside the box ...
    assert ((st & 1) == 0).all()
    assert torch.equal(spec, gen)


def _speckle(b, scene, seed):
    """The scene's own occupancy plus pixels in the first and last rows and columns of the occupancy
    window, at its bit boundaries 31/32, 63/64 and 95/96 (and one column either side, since the
    window's bit 0 follows the load alignment; these rooms' windows are 106 columns wide, so bit 127
    lies outside them), and a sparse random scatter over the whole window."""
    i0, j0, h, w = _rect(b)
    occ = np.array(scene['occupancy'][0], dtype=np.uint8)
    wi0, wj0, wh, ww = i0 - RMAX, j0 - RMAX, h + 2 * RMAX, w + 2 * RMAX
    rs = np.random.RandomState(seed)
    win = occ[wi0:wi0 + wh, wj0:wj0 + ww]
    win[rs.rand(wh, ww) < 0.0015] = 1
    rows = [0, 1, RMAX - 1, RMAX, RMAX + 1, wh // 2, wh - RMAX - 1, wh - RMAX, wh - 2, wh - 1]
    cols = [k + d for k in (0, 32, 64, 96, 128) for d in (-2, -1, 0, 1) if 0 <= k + d < ww] + [ww - 2, ww - 1]
    for n, r in enumerate(rows):
        win[r, cols[(3 * n) % len(cols)]] = 1
        win[r, cols[(3 * n + 7) % len(cols)]] = 1
    for n, c in enumerate(cols):
        win[rows[(2 * n) % len(rows)], c] = 1
    return occ


@pytest.mark.parametrize('name, want, hw', [(FLAGSHIP, 1, (44, 92)), (LARGE, 1, (92, 92)), (S2_NAME, 2, (44, 92))])
def test_dilation_table_window_edges_and_word_boundaries(S, name, want, hw):
    """44 x 92 and 92 x 92 rooms (6 and 12 output rows per wave with two sources, 11 with one: a row
    count that is no multiple of the 4-row step), radius 5 and, in the large room, 6."""
    _lib, batch, context, synthetic = S
    scenes = [synthetic.make_scene(name, 11 + e) for e in range(2)]
    b = batch.StateBatch(scenes)
    assert _rect(b)[2:] == hw
    if name == LARGE:
        assert len({r['type'] for r in scenes[0]['robots']}) == 2
    occ = np.concatenate([np.stack([_speckle(b, sc, 100 * e + a) for a in range(len(sc['robots']))])
                          for e, sc in enumerate(scenes)])
    b.set_maps(occupancy=occ)
    spec, gen, st, dbg = _both(S, b, want)
    cs = dbg['cspace'].cpu().numpy()
    print('free share per stack:', [round(float(c.mean()), 3) for c in cs], 'rounds:', (st >> 8).tolist())
    assert 0.02 < cs.mean() < 0.98
    assert torch.equal(spec, gen)


@pytest.mark.parametrize('name, want', BOTH)
def test_descriptor_clamp_posts_the_same_fault_through_an_instance(S, name, want):
    """An agent's robot index past num_robots in a serpentine room (many rounds of the round words):
    clamped, finished normally, SIMAPS_FAULT_DESCRIPTOR with `where` = (get_state, the agent) posted
    by the instance exactly as by the generic kernel."""
    _lib, batch, context, synthetic = S
    b = _batch(S, name, (7, 8), SMALL_CELLS, [lambda b, sc: _draw(b, sc, _serpentine(*_rect(b)[2:]))] * 2)
    assert _lib.lib.simaps_get_state_instance(b.cfg, 0) == want and _lib.lib.simaps_get_state_instance(b.cfg, 1) == _lib.SPEC_GENERIC
    robots, envs, ag, paths = batch.pack_descriptors(b.scenes, b.agents)
    robots = np.concatenate([robots, np.repeat(robots[:1], 8)])
    paths = np.concatenate([paths, np.repeat(paths[:1], 40, 0)])
    ag['robot'][5] = 6                                                   # 8 agents, only agent 5 is bad
    R, E, A = (batch._to_dev(x, b.device) for x in (robots, envs, ag))
    P = torch.from_numpy(paths).to(b.device)
    status = torch.zeros(b.N, dtype=torch.int32, device=b.device)
    dbg = _lib.Debug(None, None, None, status.data_ptr(), None)
    ctx = context.Context()
    try:
        got = []
        for d in (None, dbg):                                            # the instance, then the generic kernel
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
        st = status.cpu().numpy()
        assert st[5] & 8 and not (st[[0, 1, 2, 3, 4, 6, 7]] & 8).any() and (st >> 8).max() >= 7
    finally:
        torch.cuda.synchronize()
        ctx.fault_status(clear=True)
        ctx.close()


def _xy(b, row, col):
    i0, j0, h, w = _rect(b)
    return (float((j0 + col + 0.5 - b.W / 2) / 96.0), float((b.H / 2 - (i0 + row + 0.5)) / 96.0), 0)


def _with_paths(b, scene, rows):
    """Every robot of the scene active, at row rows[0] with an intention path over a waypoint to a
    target at row rows[1] (columns spread over the room)."""
    for k, r in enumerate(scene['robots']):
        c = 10 + 22 * k
        r['position'] = _xy(b, rows[0], c)
        r['waypoint_positions'] = [r['position'], _xy(b, (rows[0] + rows[1]) // 2, c + 6), _xy(b, rows[1], c + 3)]
        r['waypoint_index'] = 1
        r['target_ee'] = _xy(b, rows[1], c + 8)
        r['idle'] = False


@pytest.mark.parametrize('path', ['early', 'late'])
def test_scratch_zeroing_early_and_late(S, path):
    """The render waves of the two-source instance zero the released cspace scratch ahead of the
    barrier after the robot stamps (early, the product) or, where a wave found it still held, at the
    raster start (late: the diagnostic ring build makes every wave take that path).  Env 0: robots in
    the bottom rows with intention paths to the top rows, more than 31 pixels above them -- segments in
    the tile rows that alias the scratch (its first 1,328 16-byte words = 38.5 tile rows); env 1:
    paths within 4 rows of the robots, none there.  Instance against generic kernel of the same
    library, and the late path's stacks against the product's."""
    _lib, batch, context, synthetic = S
    scenes = [synthetic.make_scene(FLAGSHIP, 21), synthetic.make_scene(FLAGSHIP, 22)]
    b = batch.StateBatch(scenes)
    _with_paths(b, scenes[0], (38, 6))
    _with_paths(b, scenes[1], (22, 26))
    b.set_descriptors(scenes)
    b.set_maps(occupancy=np.concatenate([np.repeat(_draw(b, sc, [])[None], 4, 0) for sc in scenes]))
    spec, gen, st, dbg = _both(S, b, 1)
    assert torch.equal(spec, gen)
    ch = 4                                                              # overhead, robot, 2 x sp, intention
    assert spec.shape[1] == 5 and float(spec[:4, ch].abs().max()) > 0 and float(spec[4:, ch].abs().max()) > 0
    if path == 'early':
        return
    lib = os.path.join(os.path.dirname(_lib.__file__), 'libsimaps_diagring.so')
    if not os.path.exists(lib):
        pytest.fail('build the diagnostic library first: make -C spatial-intention-maps_amd/csrc diag')
    L = _lib._load(lib)
    assert L.simaps_fault_status(1) == 0
    status = torch.zeros(b.N, dtype=torch.int32, device=b.device)
    outs = []
    for d in (None, _lib.Debug(None, None, None, status.data_ptr(), None)):   # S1 (late path), then generic
        out = b.alloc_state()
        assert L.simaps_get_state(b.cfg, b.N, _lib.ptr(b.agents_d), _lib.ptr(b.envs_d), _lib.ptr(b.robots_d),
                                  _lib.ptr(b.paths_d), _lib.ptr(b.occupancy), _lib.ptr(b.overhead), _lib.ptr(out), 0, d,
                                  _lib.stream_handle()) == 0
        torch.cuda.synchronize()
        outs.append(out)
    assert L.simaps_fault_status(0) == 0 and ((status.cpu().numpy() & 14) == 0).all()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], spec)
