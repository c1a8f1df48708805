"""From policy outputs back to actions (the counterpart of policy_input).

The reference picks each awaiting robot's action in DQNPolicy.step (policies.py:49-66): with
probability exploration_eps a uniform draw from the robot type's action space, else the arg-max of
the network's [K, 96, 96] output, one robot at a time with a device->host `.item()` each.  Here the
epsilon draws stay on the host, through the caller's `random` in the reference's order, so that a
seeded run follows the reference's draws; the arg-max -- the only part that needs the outputs -- is
left to the device (StateBatch.store_new_actions / VectorEnvObservations.store_new_action), marked -1.

Two ways to explore, and which to use when:
  select_actions     the host draw above.  Use it when a run has to follow the reference's draws (a
                     seeded comparison with policies.py): it consumes the caller's `random` exactly as
                     DQNPolicy.step does.  It costs one host step and an upload between the policy and
                     the action call, so that step cannot be part of a captured graph.
  DeviceExploration  the draw on the device (include/simaps_action_as.h): pass exploration_eps= and
                     rng= to store_new_actions / store_new_action and leave the actions at -1.  Q maps,
                     actions, descriptors and next states are then one stream-ordered sequence that a
                     captured graph replays with fresh exploration each time.  It is a counter-based
                     Philox4x32-10 draw per agent and does NOT reproduce Python's `random` stream.
"""
import random as _random

import torch

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


class DeviceExploration:
    """The 2-word device state {seed, step} of the device exploration draw (include/simaps_action_as.h).

    Every store_new_actions / store_new_action call given this as rng= reads it on the device and
    advances step by one in a kernel of its own, so a replayed graph advances it too; the host never
    writes it after construction.  tests/explore_ref.py restates the draw."""

    def __init__(self, seed, device='cuda', step=0):
        seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
        signed = [v - 2 ** 64 if v >= 2 ** 63 else v for v in (seed, step)]  # (the words' bits, as int64)
        self.seed = seed
        self._state = torch.tensor(signed, dtype=torch.int64, device=device)

    @property
    def tensor(self):
        """The [2] int64 device tensor {seed, step} a call takes as rng."""
        return self._state

    def read_step_synchronising(self):
        """The step as the device holds it now: a SYNCHRONISING read-back (a device->host copy that
        waits for the current stream), for tests and logging, not for the training loop."""
        return int(self._state[1].item()) & (2 ** 64 - 1)

    @property
    def step(self):
        """read_step_synchronising() as a property: reading it SYNCHRONISES with the device."""
        return self.read_step_synchronising()
