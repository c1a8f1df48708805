"""A host model of get_state's per-map-slot state cache, written from include/simaps_state_cache.h
alone (not from the kernel): which calls use the cache, what a record's key is, which occupancy bits
a record compares, and which launches hit, miss or go without.  Plain numpy; no GPU.

    uses_cache(cfg)             the header's "which calls use the cache" rule for a float32 call
    key(cfg, scene, agent)      the eleven key fields of simaps_state_cache_header
    window_bits(occ, cfg)       the compared block: occ[i0-7 : i0+h+7, a0 : a0+144] != 0
    Model                       per slot nothing or (key, bits); render(slots) -> outcomes

cfg is anything with simaps_config's field names as attributes (a simaps._lib.Config, or config_of()).
"""
import types

import numpy as np

import oracle
from simaps import constants as K

MAGIC = 0x53433031                 # SIMAPS_STATE_CACHE_MAGIC
PAD = 7                            # the window's margin around the room rectangle
WIN_BYTES = 144                    # the bytes of a map row that a record compares (words 0..4)
SMALL = (184, 232, 44, 92)         # SIMAPS_ROOM_SMALL: H, W, room_h, room_w (include/simaps_spec_room.h)
KEY_FIELDS = ('magic', 'H', 'W', 'room_i0', 'room_j0', 'room_h', 'room_w', 'cspace_radius', 'has_receptacle',
              'rec_i', 'rec_j')


def config_of(scene, room_rect=None, layout_chw=True):
    """The fields of simaps_config that the model reads, for `scene` (room_rect: (i0, j0, h, w), default
    the scene's own 'room_rect' or the room's centred rectangle)."""
    f = scene['flags']
    i0, j0, h, w = room_rect or scene.get('room_rect') or K.room_rect(scene['room_width'], scene['room_length'])
    return types.SimpleNamespace(
        H=scene['H'], W=scene['W'], room_i0=i0, room_j0=j0, room_h=h, room_w=w,
        use_robot_map=int(f['use_robot_map']), use_distance_to_receptacle_map=int(f['use_distance_to_receptacle_map']),
        use_shortest_path_to_receptacle_map=int(f['use_shortest_path_to_receptacle_map']),
        use_shortest_path_map=int(f['use_shortest_path_map']), use_intention_map=int(f['use_intention_map']),
        use_history_map=int(f['use_history_map']), use_intention_channels=int(f['use_intention_channels']),
        layout_chw=int(layout_chw))


def window_a0(cfg):
    """The first map column of the compared block: the window's first column rounded down to 4 bytes."""
    return (int(cfg.room_j0) - PAD) & ~3


def uses_cache(cfg, float32=True, debug=False):
    """The header's rule: a float32 call without debug output that takes instance S1 (the two-source
    standard stack, CHW) in the small room class, whose rows allow the 4-byte window loads."""
    s1 = (cfg.use_robot_map and not cfg.use_distance_to_receptacle_map and cfg.use_shortest_path_to_receptacle_map
          and cfg.use_shortest_path_map and cfg.use_intention_map and not cfg.use_history_map
          and not cfg.use_intention_channels and cfg.layout_chw)
    small = (int(cfg.H), int(cfg.W), int(cfg.room_h), int(cfg.room_w)) == SMALL
    j0 = int(cfg.room_j0)
    return bool(float32 and not debug and s1 and small and j0 >= PAD and window_a0(cfg) + WIN_BYTES <= int(cfg.W))


def key(cfg, scene, agent):
    """The eleven key fields of the record that `agent`'s stack of `scene` writes, in KEY_FIELDS order."""
    rec = scene['receptacle_position']
    x, y = (0.0, 0.0) if rec is None else rec[:2]          # a missing receptacle packs as (0, 0)
    ri, rj = oracle.position_to_pixel_indices(x, y, (int(cfg.H), int(cfg.W)))
    return (MAGIC, int(cfg.H), int(cfg.W), int(cfg.room_i0), int(cfg.room_j0), int(cfg.room_h), int(cfg.room_w),
            int(K.cspace_radius_px(scene['robots'][agent]['type'])), int(rec is not None), int(ri), int(rj))


def window_bits(occ, cfg):
    """bool [room_h + 14, 144]: occ[i0-7 : i0+h+7, a0 : a0+144] != 0, rows outside the map 0."""
    occ = np.asarray(occ)
    H, W = occ.shape
    i0, h, a0 = int(cfg.room_i0), int(cfg.room_h), window_a0(cfg)
    assert 0 <= a0 and a0 + WIN_BYTES <= W, 'window_bits: the rule of uses_cache() does not hold'
    out = np.zeros((h + 2 * PAD, WIN_BYTES), dtype=bool)
    lo, hi = max(i0 - PAD, 0), min(i0 + h + PAD, H)
    out[lo - (i0 - PAD):hi - (i0 - PAD)] = occ[lo:hi, a0:a0 + WIN_BYTES] != 0
    return out


def window_pixel(cfg, row, col):
    """Map pixel (i, j) of the compared block's (row, col)."""
    return int(cfg.room_i0) - PAD + row, window_a0(cfg) + col


class Model:
    """Per map slot nothing or (key, bits).  inputs(slot) -> (key, bits) of the slot's current inputs.

    render(slots) -> one outcome per launched slot: 'hit' (the record equals the inputs), 'miss' (it
    does not: the record is rewritten) or 'uncached' (the launch names a slot twice, so it goes without
    the cache as a whole).  hits / misses are the records' counters."""

    def __init__(self, num_slots, inputs):
        self.inputs = inputs
        self.records = [None] * num_slots
        self.hits = [0] * num_slots
        self.misses = [0] * num_slots

    def peek(self, slot):
        """What a cached render of `slot` would be now, without rendering."""
        k, bits = self.inputs(slot)
        rec = self.records[slot]
        return 'hit' if rec is not None and rec[0] == k and np.array_equal(rec[1], bits) else 'miss'

    def render(self, slots=None):
        slots = list(range(len(self.records))) if slots is None else [int(s) for s in slots]
        if len(set(slots)) != len(slots):
            return ['uncached'] * len(slots)
        out = []
        for s in slots:
            o = self.peek(s)
            if o == 'hit':
                self.hits[s] += 1
            else:
                k, bits = self.inputs(s)
                self.records[s] = (k, bits.copy())
                self.misses[s] += 1
            out.append(o)
        return out
