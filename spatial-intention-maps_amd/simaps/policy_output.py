"""From policy outputs back to actions (the counterpart of policy_input).

The reference picks each awaiting robot's action in DQNPolicy.step (policies.py:49-66): with
probability exploration_eps a uniform draw from the robot type's action space, else the arg-max of
the network's [K, 96, 96] output, one robot at a time with a device->host `.item()` each.  Here the
epsilon draws stay on the host, through the caller's `random` in the reference's order, so that a
seeded run follows the reference's draws; the arg-max -- the only part that needs the outputs -- is
left to the device (StateBatch.store_new_actions / VectorEnvObservations.store_new_action), marked -1.
"""
import random as _random

from . import _lib
from . import constants as K


def get_num_output_channels(robot_type):
    """VectorEnv.get_num_output_channels (envs.py:371-372): Robot.NUM_OUTPUT_CHANNELS of the class."""
    n = _lib.lib.simaps_num_output_channels(_lib.TYPE_IDS.get(robot_type, robot_type) if isinstance(robot_type, str)
                                            else int(robot_type))
    if n < 0:
        raise ValueError('unknown robot type %r' % (robot_type,))
    return n


def get_action_space(robot_type):
    """VectorEnv.get_action_space (envs.py:375-376): output channels x 96 x 96."""
    return get_num_output_channels(robot_type) * K.LOCAL_MAP_PIXEL_WIDTH * K.LOCAL_MAP_PIXEL_WIDTH


def select_actions(outputs, exploration_eps=0.0, rng=None, group_sizes=None):
    """The action structure of DQNPolicy.step for one env, without reading the outputs' values.

    outputs: per group (robot indices, [n, K, 96, 96] batch or None), the structure
    policy_input.group_batches gives the states in.
    -> per group a list over the group's listed robots: a uniformly drawn action index where
    rng.random() < exploration_eps (rng.randrange over the group's action space K * 96 * 96 =
    VectorEnv.get_action_space(robot_type), policies.py:61-62), else -1 = "the arg-max, taken on the
    device".  rng: a random.Random, or None for the `random` module itself, which is what the
    reference draws from; one random() per robot, in the reference's order (group by group, robot by
    robot), and one randrange after each hit.  group_sizes (robots per group): the result is then
    the reference's full [group][robot] structure, None for the robots not listed (not awaiting an
    action), which VectorEnvObservations.store_new_action takes as it is."""
    rng = rng or _random
    out = []
    for idx, bt in outputs:
        row = []
        for _ in idx:
            row.append(rng.randrange(int(bt.shape[1]) * int(bt.shape[2]) * int(bt.shape[3]))
                       if rng.random() < exploration_eps else -1)
        if group_sizes is not None:
            full = [None] * group_sizes[len(out)]
            for j, a in zip(idx, row):
                full[j] = a
            row = full
        out.append(row)
    return out
