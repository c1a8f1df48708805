"""GPU: the room-class instances of get_state_kernel (include/simaps_spec_room.h, csrc/simaps_spec.hip:
GS_SPEC_ROOM, GS_SPEC_DIR_ROUNDS) against the generic kernel of the same build.

A render() without debug buffers of a standard stack in the small room launches the room-class twin of
S1 / S2 (StateBatch.room_class says so; kernel_instance keeps saying S1 / S2);
render(debug=alloc_debug()) is the generic kernel, which reads the room, the map shape and the sweep
directions at run time.  The two states must be torch.equal.  Every case renders
1 to 4 stacks (the descriptor clamp needs 8 agents to have a good one beside the bad one).

The synthetic scenes have no small room with columns of their own, so that case draws four square
columns into the flagship's room.  Hand-made rooms are drawn into the occupancy maps with set_maps, in
room-rect pixels (the recipe of tests/test_gpu_sweepdiet.py); with a configuration-space radius of 5 a
one-pixel wall blocks 11 columns / rows.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FLAGSHIP = 'lifting_4-small_divider'
S2_NAME = 'rescue_4-small_empty'
LARGE = 'pushing_4-large_empty'
SMALL = 1                                      # SIMAPS_ROOM_SMALL


@pytest.fixture(scope='module')
def S():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a GPU (run with -m gpu on an MI355X)')
    from simaps import _lib, batch, context, synthetic
    _lib.lib.simaps_fault_status(1)
    yield _lib, batch, context, synthetic
    _lib.lib.simaps_fault_status(1)


def _both(S, b, want, room, slots=None):
    """(instance render, generic render, debug outputs) of batch b, which must take instance `want`
    in room class `room`."""
    _lib = S[0]
    assert (b.kernel_instance(), b.room_class()) == (want, room)
    assert (b.kernel_instance(debug=True), b.room_class(debug=True)) == (_lib.SPEC_GENERIC, _lib.ROOM_NONE)
    n = b.N if slots is None else len(slots)
    assert n <= 4
    dbg = b.alloc_debug(n)
    spec = b.render(slots=slots)
    gen = b.render(debug=dbg, slots=slots)
    torch.cuda.synchronize()
    _lib.check_faults()
    st = dbg['status'].cpu().numpy()
    assert ((st & 14) == 0).all()                                        # no round cap, timeout or clamp
    assert spec.dtype == torch.float32 and tuple(spec.shape) == b.out_shape(n)
    return spec, gen, dbg


def _rect(b):
    c = b.cfg
    return int(c.room_i0), int(c.room_j0), int(c.room_h), int(c.room_w)


def _xy(b, row, col):
    i0, j0, h, w = _rect(b)
    return (float((j0 + col + 0.5 - b.W / 2) / 96.0), float((b.H / 2 - (i0 + row + 0.5)) / 96.0), 0)


def _place(b, scene, cells):
    """Robot k of the scene onto room-rect cell cells[k] (row, column): the centre of that pixel."""
    for r, (row, col) in zip(scene['robots'], cells):
        r['position'] = _xy(b, row, col)
        r['waypoint_positions'] = [r['position']] + list(r['waypoint_positions'][1:])


def _draw(b, scene, walls, open_map=False):
    """The scene's occupancy with the room interior cleared (open_map: the whole map, so that the
    room's first and last rows and columns are free too) and `walls` drawn, each (row0, row1, col0,
    col1) inclusive in room-rect pixels."""
    i0, j0, h, w = _rect(b)
    occ = np.array(scene['occupancy'][0], dtype=np.uint8)
    if open_map:
        occ[:] = 0
    occ[i0:i0 + h, j0:j0 + w] = 0
    for r0, r1, c0, c1 in walls:
        occ[i0 + r0:i0 + r1 + 1, j0 + c0:j0 + c1 + 1] = 1
    return occ


def _box(r0, r1, c0, c1):
    return [(r0, r0, c0, c1), (r1, r1, c0, c1), (r0, r1, c0, c0), (r0, r1, c1, c1)]


def _one_env(S, name, seed, cells=None, walls=None, open_map=False, rounding='fma', receptacle=None):
    """StateBatch of one env of `name` (4 stacks): robots on `cells`, the room redrawn with `walls`."""
    _lib, batch, context, synthetic = S
    scene = synthetic.make_scene(name, seed)
    scene['rotate_rounding'] = rounding
    b = batch.StateBatch([scene])
    assert b.N == 4 and b.cfg.rotate_rounding == _lib.ROT_IDS[rounding]
    if cells is not None:
        _place(b, scene, cells)
    if receptacle is not None:
        scene['receptacle_position'] = _xy(b, *receptacle)
    if cells is not None or receptacle is not None:
        b.set_descriptors([scene])
    if walls is not None:
        b.set_maps(occupancy=np.repeat(_draw(b, scene, walls, open_map)[None], 4, 0))
    return b


COLUMNS = _box(12, 15, 20, 23) + _box(28, 31, 34, 37) + _box(12, 15, 56, 59) + _box(28, 31, 70, 73)
MATCHING = [(FLAGSHIP, 1, None), (S2_NAME, 2, None), (FLAGSHIP, 1, COLUMNS)]


@pytest.mark.parametrize('rounding', ['fma', 'plain'])
@pytest.mark.parametrize('name, want, walls', MATCHING, ids=['divider', 'rescue_empty', 'columns'])
def test_room_instance_equals_generic_with_4_agents_and_with_1(S, name, want, walls, rounding):
    """The scene as synthetic makes it (or the flagship's room with four columns drawn in): the whole
    env in one launch, then each of two agents in a launch of its own."""
    b = _one_env(S, name, 3, walls=walls, rounding=rounding)
    assert _rect(b)[2:] == (44, 92)
    spec, gen, dbg = _both(S, b, want, SMALL)
    assert torch.equal(spec, gen)
    assert not torch.isnan(spec).any() and float(spec.abs().max()) > 0
    nsrc = (dbg['sources'][:, :, 0] >= 0).sum(1).cpu().numpy()
    assert (nsrc == (2 if want == 1 else 1)).all()
    for k in (0, 3):
        one, gen1, _ = _both(S, b, want, SMALL, slots=[k])
        assert torch.equal(one, gen1) and torch.equal(one[0], spec[k])


def test_plain_rounding_on_another_scene(S):
    """rotate_rounding is a run-time value of the room instances: the plain form on a second scene."""
    b = _one_env(S, FLAGSHIP, 5, rounding='plain')
    spec, gen, _ = _both(S, b, 1, SMALL)
    assert torch.equal(spec, gen)


def _off_by(S, name, field, delta):
    """One env of `name` with the configuration's `field` changed by delta cells (the maps stay what
    they were: the room rect is just read one cell smaller or larger)."""
    b = _one_env(S, name, 4)
    setattr(b.cfg, field, getattr(b.cfg, field) + delta)
    return b


@pytest.mark.parametrize('name, want', [(FLAGSHIP, 1), (S2_NAME, 2)])
@pytest.mark.parametrize('field, delta', [('room_h', 1), ('room_h', -1), ('room_w', -1), ('room_w', 1)])
def test_one_cell_off_takes_s1_s2_and_stays_exact(S, name, want, field, delta):
    """45 and 43 rows; 91 columns (pitch 93: the run-time-pitch sweeps) and 93 (pitch 95 still)."""
    _lib = S[0]
    b = _off_by(S, name, field, delta)
    spec, gen, _ = _both(S, b, want, _lib.ROOM_NONE)
    assert torch.equal(spec, gen) and float(spec.abs().max()) > 0


def test_large_room_takes_s1_and_stays_exact(S):
    _lib = S[0]
    b = _one_env(S, LARGE, 2)
    assert _rect(b)[2:] == (92, 92)
    spec, gen, _ = _both(S, b, 1, _lib.ROOM_NONE)
    assert torch.equal(spec, gen)


# ---- sweep edge cases: the smallest shapes where bounds folded from 44 x 92 can go wrong

EDGE_CELLS = [(0, 30), (43, 60), (20, 0), (25, 91)]      # first row, last row, first column, last column


@pytest.mark.parametrize('name, want', [(FLAGSHIP, 1), (S2_NAME, 2)])
@pytest.mark.parametrize('open_map', [True, False], ids=['open', 'walled'])
def test_sources_on_the_rooms_first_and_last_rows_and_columns(S, name, want, open_map):
    """Each agent's robot on another edge line of the room.  open: no obstacle anywhere in the map, so
    the edge cells are free and each source is its own pixel, on dirty line 0 / len - 1 of a direction
    (the receptacle in a corner: two of them at once).  walled: the walls around the room stand, the edge
    lines are outside the configuration space and each source is snapped inwards."""
    b = _one_env(S, name, 6, cells=EDGE_CELLS, walls=[], open_map=open_map, receptacle=(0, 91))
    spec, gen, dbg = _both(S, b, want, SMALL)
    i0, j0, h, w = _rect(b)
    src = dbg['sources'].cpu().numpy()
    rob = src[:, 1] - np.array([i0, j0, i0, j0])
    print('robot sources (query, snapped), room cells:', rob.tolist())
    assert [tuple(r[:2]) for r in rob.tolist()] == EDGE_CELLS
    snapped = (src[:, 1, :2] != src[:, 1, 2:]).any(1)
    assert snapped.all() != open_map and snapped.any() != open_map
    if open_map:
        assert dbg['cspace'].all()
    assert ((dbg['status'].cpu().numpy() & 1) == 0).all()
    assert torch.equal(spec, gen)


@pytest.mark.parametrize('name, want', [(FLAGSHIP, 1), (S2_NAME, 2)])
def test_walled_in_source_with_no_other_reachable_cell(S, name, want):
    """Robot 0 in the middle of a closed 13 x 13 box: inside, only its own pixel is outside the
    dilated walls, so its source reaches no other cell (the maximum pass finds the source's 0 alone)
    and every sweep of that array ends in its first round; the other robots stand outside."""
    box = _box(10, 22, 60, 72)
    b = _one_env(S, name, 8, cells=[(16, 66), (30, 10), (36, 30), (8, 20)], walls=box)
    spec, gen, dbg = _both(S, b, want, SMALL)
    cs = dbg['cspace'].cpu().numpy()[0].astype(bool)
    assert cs[16, 66] and cs[10:23, 60:73].sum() == 1
    src = dbg['sources'].cpu().numpy()
    assert (src[0, 1, :2] == src[0, 1, 2:]).all()                        # not snapped: its own pixel
    d = dbg['dist'].cpu().numpy()[0, 1]
    print('cells the walled-in source reaches:', int((d >= 0).sum()), 'rounds:', (dbg['status'].cpu().numpy() >> 8).tolist())
    assert (d >= 0).sum() == 1 and d[16, 66] == 0                # (the debug dump writes -1 for unreachable)
    assert torch.equal(spec, gen)


DIVIDERS = {'column_short_of_both': (1, 42, 46, 46), 'column_short_of_top': (1, 43, 46, 46),
            'row_short_of_both': (22, 22, 1, 90), 'row_short_of_right': (22, 22, 0, 90)}


@pytest.mark.parametrize('divider', sorted(DIVIDERS))
def test_divider_one_cell_short_of_a_wall(S, divider):
    """A one-pixel divider across the room that stops one cell before the wall(s): on an open map
    (no walls around the room) the one-cell gap stays blocked by the divider's own dilation, so the
    far side is unreachable except around the room's outside, which the room rect cuts off."""
    b = _one_env(S, FLAGSHIP, 9, cells=[(10, 10), (34, 20), (36, 80), (8, 70)], walls=[DIVIDERS[divider]],
                 open_map=True)
    spec, gen, dbg = _both(S, b, 1, SMALL)
    d = dbg['dist'].cpu().numpy()[:, 1]
    print('cells each robot source reaches:', (d >= 0).reshape(4, -1).sum(1).tolist())
    assert not (d >= 0).reshape(4, -1).all(1).any()                # some cell is cut off for every agent
    assert torch.equal(spec, gen)


@pytest.mark.parametrize('name, want', [(FLAGSHIP, 1), (S2_NAME, 2)])
def test_descriptor_clamp_posts_the_same_fault_through_a_room_instance(S, name, want):
    """An agent's robot index past num_robots (the recipe of tests/test_gpu_spec.py): the room-class
    instance clamps it, finishes normally and posts SIMAPS_FAULT_DESCRIPTOR with `where` =
    (get_state, the agent) exactly as the generic kernel does."""
    _lib, batch, context, synthetic = S
    b = batch.StateBatch([synthetic.make_scene(name, 7 + e) for e in range(2)])
    robots, envs, ag, paths = batch.pack_descriptors(b.scenes, b.agents)
    robots = np.concatenate([robots, np.repeat(robots[:1], 8)])
    paths = np.concatenate([paths, np.repeat(paths[:1], 40, 0)])
    ag['robot'][5] = 6                                                   # 8 agents, only agent 5 is bad
    R, E, A = (batch._to_dev(x, b.device) for x in (robots, envs, ag))
    P = torch.from_numpy(paths).to(b.device)
    status = torch.zeros(b.N, dtype=torch.int32, device=b.device)
    dbg = _lib.Debug(None, None, None, status.data_ptr(), None)
    assert _lib.lib.simaps_get_state_instance(b.cfg, 0) == want
    assert _lib.lib.simaps_get_state_room_class(b.cfg, 0) == SMALL
    assert _lib.lib.simaps_get_state_room_class(b.cfg, 1) == _lib.ROOM_NONE
    ctx = context.Context()
    try:
        got = []
        for d in (None, dbg):                                            # the room instance, then the generic kernel
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
