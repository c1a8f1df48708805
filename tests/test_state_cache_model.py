"""CPU: the host model of the state cache (tests/state_cache_model.py), the oracle's room rectangle
argument, and the scripted episodes of tests/state_cache_episodes.py, which the GPU tests replay
(tests/test_gpu_state_cache_episodes.py).  Nothing here needs a GPU."""
import numpy as np
import pytest

import goldens
import oracle
import state_cache_episodes as EP
import state_cache_model as M
from simaps import constants as K
from simaps import synthetic

FLAGSHIP = 'lifting_4-small_divider'


def test_oracle_room_rect_default_is_the_room_mask_bit_for_bit():
    cases = [c for c in goldens.scene_cases() if c[0] == FLAGSHIP]        # the golden flagship scene's agents
    assert cases
    for _, _, a, scene, pre, z in cases:
        rect = K.room_rect(scene['room_width'], scene['room_length'])
        assert rect == (70, 70, 44, 92)
        want, got = oracle.agent_state(scene, a), oracle.agent_state(dict(scene, room_rect=rect), a)
        assert want.dtype == np.float32 and np.array_equal(want.view(np.uint32), got.view(np.uint32))
        assert np.array_equal(got.view(np.uint32), z[pre + 'state'].view(np.uint32))
    scene = synthetic.make_scene(FLAGSHIP, 0)
    # and another rectangle is another mask
    moved = oracle.AgentOracle(dict(scene, room_rect=(68, 72, 44, 92)), 0)
    assert moved.cspace[:68].sum() == 0 and moved.cspace[:, :72].sum() == 0 and moved.cspace[68:112, 72:164].sum() > 0
    assert moved.cspace[112:].sum() == 0 and moved.cspace[:, 164:].sum() == 0


def test_uses_cache_follows_the_header_rule():
    scene = synthetic.make_scene(FLAGSHIP, 0)
    on = {(70, 70), (70, 7), (70, 98), (3, 70), (137, 70), (70, 68), (70, 69), (70, 71), (70, 72)}
    off = {(70, 6), (70, 99), (0, 0), (140, 140)}
    for i0, j0 in sorted(on | off):
        assert M.uses_cache(M.config_of(scene, (i0, j0, 44, 92))) == ((i0, j0) in on), (i0, j0)
    c = M.config_of(scene)
    assert not M.uses_cache(c, float32=False) and not M.uses_cache(c, debug=True)
    assert not M.uses_cache(M.config_of(scene, layout_chw=False))
    assert not M.uses_cache(M.config_of(synthetic.make_scene('pushing_4-large_empty', 0)))
    assert not M.uses_cache(M.config_of(synthetic.make_scene('lifting_4-small_divider-history', 0)))
    assert [(M.window_a0(M.config_of(scene, (70, j, 44, 92))), (j - 7) & 3) for j in (68, 69, 70, 71, 72, 98)] == \
        [(60, 1), (60, 2), (60, 3), (64, 0), (64, 1), (88, 3)]


def test_key_fields():
    scene = synthetic.make_scene(FLAGSHIP, 0)
    c = M.config_of(scene)
    k = dict(zip(M.KEY_FIELDS, M.key(c, scene, 2)))
    ri, rj = oracle.position_to_pixel_indices(scene['receptacle_position'][0], scene['receptacle_position'][1], (184, 232))
    assert len(M.KEY_FIELDS) == 11 and k == dict(magic=0x53433031, H=184, W=232, room_i0=70, room_j0=70, room_h=44, room_w=92,
                                                 cspace_radius=5, has_receptacle=1, rec_i=ri, rec_j=rj)
    none = dict(scene, receptacle_position=None)
    k = dict(zip(M.KEY_FIELDS, M.key(c, none, 2)))
    assert (k['has_receptacle'], k['rec_i'], k['rec_j']) == (0, 92, 116)      # (0.0, 0.0): the map's centre pixel
    scene['robots'][2]['type'] = 'pushing_robot'
    assert dict(zip(M.KEY_FIELDS, M.key(c, scene, 2)))['cspace_radius'] == 6
    assert dict(zip(M.KEY_FIELDS, M.key(c, scene, 1)))['cspace_radius'] == 5


def test_window_bits_block_and_its_four_sides():
    scene = synthetic.make_scene(FLAGSHIP, 0)
    c = M.config_of(scene)
    occ = scene['occupancy'][0].copy()
    base = M.window_bits(occ, c)
    assert base.shape == (58, 144) and base.dtype == bool and base.any()
    r0, r1, c0, c1 = 63, 63 + 57, 60, 60 + 143                              # the block's first and last row and column
    assert M.window_pixel(c, 0, 0) == (r0, c0) and M.window_pixel(c, 57, 143) == (r1, c1)

    def flipped(i, j):
        o = occ.copy()
        o[i, j] = 0 if o[i, j] else 1
        return M.window_bits(o, c)

    for (i, j), (wr, wc) in zip([(r0, c0), (r0, c1), (r1, c0), (r1, c1)], [(0, 0), (0, 143), (57, 0), (57, 143)]):
        d = flipped(i, j) != base
        assert d.sum() == 1 and d[wr, wc]
    for i, j in [(r0 - 1, 100), (r1 + 1, 100), (90, c0 - 1), (90, c1 + 1)]:
        assert np.array_equal(flipped(i, j), base)
    o = occ.copy()
    o[o != 0] = 0x80                                                          # any nonzero byte is a set bit
    assert np.array_equal(M.window_bits(o, c), base)
    # rows outside the map read 0
    top = M.window_bits(np.ones((184, 232), np.uint8), M.config_of(scene, (3, 70, 44, 92)))
    assert not top[:4].any() and top[4:].all()
    bot = M.window_bits(np.ones((184, 232), np.uint8), M.config_of(scene, (137, 70, 44, 92)))
    assert bot[:54].all() and not bot[54:].any()


def test_model_a_b_a():
    """Map A -> B -> A: with a render at B two misses; with the slot left out of the launch while it
    holds B, the next render hits.  A launch that names a slot twice goes without the cache."""
    scene = synthetic.make_scene(FLAGSHIP, 0)
    c = M.config_of(scene)
    occ = [scene['occupancy'][a].copy() for a in range(4)]
    m = M.Model(4, lambda s: (M.key(c, scene, s), M.window_bits(occ[s], c)))
    assert m.render() == ['miss'] * 4 and m.render() == ['hit'] * 4
    a = occ[1].copy()
    b = a.copy()
    b[90, 100] ^= 1
    occ[1] = b
    assert m.render([3, 1]) == ['hit', 'miss']
    occ[1] = a
    assert m.render() == ['hit', 'miss', 'hit', 'hit']                        # rendered at B: two misses
    occ[2] = b
    assert m.render([0, 1, 3]) == ['hit'] * 3                                 # slot 2 holds B and is not rendered
    occ[2] = scene['occupancy'][2].copy()
    assert m.render() == ['hit'] * 4                                          # A again: its record never saw B
    assert m.render([1, 1]) == ['uncached'] * 2
    assert (m.hits, m.misses) == ([4, 3, 3, 5], [1, 3, 1, 1])                   # (slot 0: 4 of 5 cached launches after its first)
    scene['receptacle_position'] = None
    assert m.render([0]) == ['miss'] and m.peek(1) == 'miss' and m.peek(0) == 'hit'


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_episode_scripts_cover_every_operation(seed):
    """The generator and the model alone: every operation occurs, and the model's outcome of every
    launch is what the operations promise (Episode.launch asserts it)."""
    ep = EP.Episode(seed)
    launches = 0
    for st in ep.steps():
        for slots in st.launches:
            ep.launch(st, slots)
            launches += 1
    totals = ep.finish()
    assert len(ep.plan) == EP.STEPS and launches == EP.STEPS + 1
    assert totals['hits'] > 0 and totals['misses'] >= ep.N
    print(totals, sorted('0x%02x' % v for v in ep.byte_values))


def test_episode_byte_values_cover_all_eight_over_the_seeds():
    seen = set()
    for seed in (0, 1, 2):
        ep = EP.Episode(seed)
        for st in ep.steps():
            for slots in st.launches:
                ep.launch(st, slots)
        seen |= ep.byte_values
    assert seen == set(EP.BYTE_VALUES)


def test_episode_oracle_runs_on_what_the_script_leaves():
    """The oracle renders the first and the last launch of seed 0 without raising."""
    ep = EP.Episode(0)
    for st in ep.steps():
        for slots in st.launches:
            ep.launch(st, slots)
        if st.k in (0, EP.STEPS - 1):
            for s in st.launches[0]:
                e, a = ep.agents[s]
                out = oracle.agent_state(ep.scenes[e], a)
                assert out.shape == (96, 96, 5) and np.isfinite(out).all()
