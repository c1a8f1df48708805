"""Robot.store_new_action (envs.py:857-903) restated in numpy / math on top of a GIVEN movement path,
and the loader of tests/golden/actions.npz (written by tests/golden/make_action_goldens.py from the
reference itself).  tests/test_action_abi.py pins this restatement to every fixture case; the GPU
tests then use it where no fixture exists (fresh scenes)."""
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
W = 96                       # Mapper.LOCAL_MAP_PIXEL_WIDTH
PPM = 96.0                   # Mapper.LOCAL_MAP_PIXELS_PER_METER
CUBE_WIDTH = 0.044           # VectorEnv.CUBE_WIDTH
BACKPACK_OFFSET = -0.0135    # Robot.BACKPACK_OFFSET
BASE_LENGTH = 0.065
# END_EFFECTOR_LOCATION per class id (lifting, pushing, throwing, rescue; envs.py:807, 1061, 1281)
END_EFFECTOR = [BACKPACK_OFFSET + BASE_LENGTH, BACKPACK_OFFSET + (BASE_LENGTH + 0.005),
                BACKPACK_OFFSET + (BASE_LENGTH + 0.006), BACKPACK_OFFSET + BASE_LENGTH]
NUM_OUTPUT_CHANNELS = [2, 1, 2, 2]
TYPE_IDS = {'lifting_robot': 0, 'pushing_robot': 1, 'throwing_robot': 2, 'rescue_robot': 3}


def restrict_heading_range(h):
    return (h + math.pi) % (2 * math.pi) - math.pi


def action_tuple(action, robot_type):
    return tuple(int(v) for v in np.unravel_index(int(action), (NUM_OUTPUT_CHANNELS[robot_type], W, W)))


def target(action, robot_type, position, heading):
    """envs.py:859-869: target_end_effector_position[:2]."""
    _, row, col = action_tuple(action, robot_type)
    dx = ((col + 0.5) - W / 2) / PPM
    dy = (W / 2 - (row + 0.5)) / PPM
    dist = math.sqrt(dx ** 2 + dy ** 2)
    theta = heading + math.atan2(-dx, dy)
    return (position[0] + dist * math.cos(theta), position[1] + dist * math.sin(theta))


def finish(path, robot_type, heading):
    """envs.py:880-903 on `path` (the waypoints before the offset, [n, 2]): (waypoints [n, 2],
    headings [n], signed_dist)."""
    wp = [(float(p[0]), float(p[1])) for p in path]
    hd = [heading]
    for i in range(1, len(wp)):
        hd.append(restrict_heading_range(math.atan2(wp[i][1] - wp[i - 1][1], wp[i][0] - wp[i - 1][0])))
    signed_dist = math.sqrt((wp[-1][0] - wp[-2][0]) ** 2 + (wp[-1][1] - wp[-2][1]) ** 2) - \
        (END_EFFECTOR[robot_type] + CUBE_WIDTH / 2)
    wp[-1] = (wp[-2][0] + signed_dist * math.cos(hd[-1]), wp[-2][1] + signed_dist * math.sin(hd[-1]))
    if len(wp) > 2 and signed_dist < 0:
        wp[-2] = wp[-1]
        hd[-2] = restrict_heading_range(math.atan2(wp[-2][1] - wp[-3][1], wp[-2][0] - wp[-3][0]))
    return np.array(wp, dtype=np.float64), np.array(hd, dtype=np.float64), signed_dist


def angle_diff(a, b):
    """|a - b| as an angle (headings near +-pi may differ by 2 pi in the last bit)."""
    d = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) % (2 * math.pi)
    return np.minimum(d, 2 * math.pi - d)


_CASES = None


def load_cases():
    """The fixture as a list of dicts (loaded once, shared, read-only): config, seed, agent, action,
    type, tuple, target, path (pre-offset), wp, hd and, for some, wp_nospm / hd_nospm."""
    global _CASES
    if _CASES is None:
        z = np.load(os.path.join(HERE, 'golden', 'actions.npz'))
        z = {k: z[k] for k in z.files}
        off = z['off']
        _CASES = []
        for c in range(len(z['action'])):
            s = slice(int(off[c]), int(off[c + 1]))
            d = {'config': str(z['configs'][z['cfg'][c]]), 'seed': int(z['seed'][c]), 'agent': int(z['agent'][c]),
                 'action': int(z['action'][c]), 'type': int(z['type'][c]), 'tuple': tuple(int(v) for v in z['tuple'][c]),
                 'target': z['target'][c], 'path': z['path'][s], 'wp': z['wp'][s], 'hd': z['hd'][s]}
            if z['has_nospm'][c]:
                d['wp_nospm'], d['hd_nospm'] = z['wp_nospm'][c], z['hd_nospm'][c]
            for v in d.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
            _CASES.append(d)
    return _CASES


OBSERVE_ALL = ('lifting_4-large_doors', 'lifting_4-large_tunnels', 'lifting_4-large_rooms')


def make_scene(synthetic, config, seed):
    """The scene a fixture case was drawn on (make_action_goldens.CONFIGS)."""
    return synthetic.make_scene(config, seed, observe_all=True) if config in OBSERVE_ALL else synthetic.make_scene(config, seed)
