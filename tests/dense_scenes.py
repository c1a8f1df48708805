"""Shared scene builders of the descriptor-limit tests (tests/test_dense_scenes.py on the CPU,
tests/test_gpu_dense.py on the GPU, tests/golden/make_goldens.py gen_dense for the fixtures): scenes
AT the limits the get_state kernels size their LDS tables for -- SIMAPS_MAX_ROBOTS = 8 robots per env
and SIMAPS_MAX_PATH = 16 points per path, i.e. all 8 x 15 = 120 segment slots -- which no scene of
simaps.synthetic, no other golden and no reference config reaches (at most 4 robots, 11 waypoints).

A case is two envs of one configuration, built on synthetic.reference_config_scene (any robot_config)
with every robot's controller state overwritten by the rules of synthetic.intention_path /
history_path: n waypoints and waypoint_index 1 give an intention path of n points, waypoint_index
n - 1 a history path of n points; 30 waypoints and index 15 give 16 points of each.

With the ramp encoding a pixel is lit only while the scaled path length stays below 1
(envs.py:2335 clips the ramp to 0), so the dense ramp cases set intention_map_scale small enough for
the last segments of a 16-point path to stay visible; tests/test_dense_scenes.py checks that they do.

Pure numpy (no torch): the python3.9 golden generator imports this module.
"""
import collections
import functools

import numpy as np

from simaps import constants as K

MAX_ROBOTS, MAX_PATH = 8, 16
SEG_PER_ROBOT = MAX_PATH - 1

# instance / room: what StateBatch.kernel_instance() / room_class() report for a render() of the case
# without debug outputs in the default chw layout (include/simaps_spec.h, include/simaps_spec_room.h)
GENERIC, S1, S2 = 0, 1, 2
ROOM_NONE, ROOM_SMALL = 0, 1

Case = collections.namedtuple('Case', 'name env_name robot_config flags seed wp lengths idle place instance room')


def _case(name, env_name, robot_config, flags, seed, instance, room, wp=(MAX_PATH, 1), lengths=None, idle=None,
          place=None):
    return Case(name, env_name, robot_config, dict(K.DEFAULT_FLAGS, **flags), seed, wp, lengths, idle, place, instance,
                room)


_S1 = {'use_intention_map': True}
_S2 = {'use_intention_map': True, 'use_shortest_path_to_receptacle_map': False}
_SPATIAL = {'use_intention_map': True, 'use_intention_channels': True, 'intention_channel_encoding': 'spatial'}


def _ties(x0, y0, d1, d2):
    """Positions of robots 0..6 (robot 7 keeps its random one).  Every number is a multiple of 1/32, so
    the differences and their squares are exact in fp64 and equal offsets give bit-equal distances:
    from robot 0, robots 1 and 6 lie at d1, robots 2, 4 and 5 at d2 and robot 3 at 0; from robot 1,
    robots 2 and 4 both lie at sqrt(d1^2 + d2^2)."""
    return [(x0, y0), (x0 + d1, y0), (x0, y0 + d2), (x0, y0), (x0, y0 - d2), (x0 - d2, y0), (x0 - d1, y0)]


# per env: robot 0 on a pixel corner ((j - W / 2) / 96, (H / 2 - i) / 96 for integers i, j)
_TIES_PLACE = ([_ties(6 / 96, -3 / 96, 12 / 96, 24 / 96), _ties(-9 / 96, 6 / 96, 9 / 96, 18 / 96)])
_TIES = {'use_intention_channels': True, 'intention_channel_encoding': 'nonspatial'}
_LIFT8 = [{'lifting_robot': 8}]

CASES = collections.OrderedDict((c.name, c) for c in [
    # S1 room-class instance, all 120 slots
    _case('s1_small_8', 'small_divider', _LIFT8, dict(_S1, intention_map_scale=0.08), 7100, S1, ROOM_SMALL),
    # plain S1 instance, segments longer than 64 px (several chunks per slot)
    _case('s1_large_8', 'large_empty', [{'pushing_robot': 8}], dict(_S1, intention_map_scale=0.04), 7110, S1, ROOM_NONE),
    # S2 room class (rescue: no receptacle maps)
    _case('s2_small_8', 'small_empty', [{'rescue_robot': 8}], dict(_S2, intention_map_scale=0.08), 7120, S2, ROOM_SMALL),
    # the generic kernel with both raster passes (the params-phase table for the history pass, then
    # seg_table for the intention pass), C = 21, robot groups 2 and 3
    _case('all_8x4groups', 'small_divider',
          [{'lifting_robot': 2}, {'pushing_robot': 2}, {'throwing_robot': 2}, {'lifting_robot': 2}],
          {'use_distance_to_receptacle_map': True, 'use_history_map': True, 'use_intention_map': True,
           'use_intention_channels': True, 'intention_channel_encoding': 'nonspatial', 'intention_map_scale': 0.08},
          7130, GENERIC, ROOM_NONE, wp=(2 * MAX_PATH - 2, MAX_PATH - 1)),
    # robot 4's slots 60..74 across the lane-64 boundary; odd robot counts
    _case('spatial_5', 'small_divider', [{'lifting_robot': 5}], dict(_SPATIAL, intention_map_scale=0.08), 7140,
          GENERIC, ROOM_NONE),
    _case('spatial_7', 'large_empty', [{'lifting_robot': 7}], dict(_SPATIAL, intention_map_scale=0.04), 7150,
          GENERIC, ROOM_NONE),
    # binary lines light every pixel at any path length: from the upper slots into the tile halo
    _case('binary_t1_8', 'small_divider', _LIFT8,
          dict(_S1, intention_map_encoding='binary', intention_map_line_thickness=1), 7160, S1, ROOM_SMALL),
    _case('binary_t2_8', 'small_divider', _LIFT8,
          dict(_S1, intention_map_encoding='binary', intention_map_line_thickness=2), 7170, S1, ROOM_SMALL),
    # line: slot 15 k of robot k alone (75, 90, 105 in the upper half, empty slots between); circle: no slot
    _case('line_8', 'small_divider', _LIFT8, dict(_S1, intention_map_encoding='line'), 7180, S1, ROOM_SMALL),
    _case('circle_8', 'small_empty', _LIFT8, dict(_S1, intention_map_encoding='circle'), 7198, S1, ROOM_SMALL),
    # empty and full slot ranges interleaved
    _case('ragged_8', 'small_divider', _LIFT8, dict(_S1, intention_map_scale=0.08), 7200, S1, ROOM_SMALL,
          lengths=[16, 2, 16, 3, 2, 16, 9, 16], idle=[(), (2, 5)]),
    # distance ties for the intention channels' order
    _case('ties_8', 'large_empty', _LIFT8, _TIES, 7210, GENERIC, ROOM_NONE, place=_TIES_PLACE),
    _case('ties_8_spatial', 'large_empty', _LIFT8, dict(_TIES, intention_channel_encoding='spatial'), 7220,
          GENERIC, ROOM_NONE, place=_TIES_PLACE),
])
CASE_IDS = list(CASES)
ENVS = 2
GOLDEN_CASES = ('s1_small_8', 'all_8x4groups', 'spatial_5', 'ties_8')
# the cases whose every robot carries a full path (the "limits reached" conditions)
FULL_CASES = ('s1_small_8', 's1_large_8', 's2_small_8', 'all_8x4groups', 'binary_t1_8', 'binary_t2_8')


def config_name(name):
    return 'dense_' + name


def _densify(case, scene, e):
    """Overwrite every robot's controller state in place; the draws come after the scene's own."""
    from simaps import synthetic
    rs = np.random.RandomState(case.seed + 1000 + e)
    L, W = scene['room_length'], scene['room_width']
    n_wp, idx = case.wp
    for k, r in enumerate(scene['robots']):
        if case.place is not None and k < len(case.place[e]):
            r['position'] = (float(case.place[e][k][0]), float(case.place[e][k][1]), 0)
        n = n_wp if case.lengths is None else case.lengths[k]
        r['waypoint_positions'] = [r['position']] + [synthetic._random_position(rs, L, W, 0.05) + (0,)
                                                     for _ in range(n - 1)]
        r['waypoint_index'] = idx
        r['idle'] = case.idle is not None and k in case.idle[e]
        if r['type'] == 'lifting_robot':
            r['lift_state'] = 'lifting' if k % 3 == 1 else 'ready'
    assert len(scene['robots']) <= MAX_ROBOTS


def build(name, e):
    """Env e of case `name`: a fresh scene dict (rotate_rounding 'fma', as synthetic makes it)."""
    from simaps import synthetic
    case = CASES[name]
    row = {'config': config_name(name), 'env_name': case.env_name, 'robot_config': case.robot_config,
           'flags': case.flags}
    scene = synthetic.reference_config_scene(row, e, seed_base=case.seed)
    _densify(case, scene, e)
    return scene


@functools.lru_cache(maxsize=None)
def _scenes(name):
    return tuple(build(name, e) for e in range(ENVS))


def scenes(name, rounding=None):
    """The case's two envs, built once per process and shared: treat them as read-only (with_idle
    copies).  rounding: 'fma' / 'plain' overrides the scenes' rotate rounding (shallow copies)."""
    sc = _scenes(name)
    return [s if rounding is None else dict(s, rotate_rounding=rounding) for s in sc]


def with_idle(scene, robots):
    """A copy of `scene` with `robots` made idle (the maps are shared)."""
    out = dict(scene)
    out['robots'] = [dict(r, idle=True) if k in robots else dict(r) for k, r in enumerate(scene['robots'])]
    return out


def path_passes(flags):
    """The raster passes of a configuration in channel order: 'history' and / or the intention encoding."""
    return (['history'] if flags['use_history_map'] else []) + \
        ([flags['intention_map_encoding']] if flags['use_intention_map'] else [])


def path_channels(flags):
    """Channel index of each pass of path_passes(flags) in the state stack (envs.py:2071-2113)."""
    c = 1 + sum(bool(flags[k]) for k in ('use_robot_map', 'use_distance_to_receptacle_map',
                                         'use_shortest_path_to_receptacle_map', 'use_shortest_path_map'))
    return list(range(c, c + len(path_passes(flags))))


def pass_points(robot, enc):
    """Points of the path a robot contributes to pass `enc` (what the kernel's segment table holds:
    one slot per consecutive pair)."""
    from simaps import synthetic
    if enc == 'circle':
        return 0
    n = len(synthetic.history_path(robot) if enc == 'history' else synthetic.intention_path(robot))
    return min(n, 2) if enc == 'line' else n


def used_slots(scene, agent, enc):
    """Segment slots q = 15 k + i that pass `enc` fills for `agent` (the other robots that are not idle)."""
    out = []
    for k, r in enumerate(scene['robots']):
        if k != agent and not r['idle']:
            out += [SEG_PER_ROBOT * k + i for i in range(max(pass_points(r, enc) - 1, 0))]
    return out
