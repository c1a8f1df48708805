"""Per-phase timing of get_state_kernel from the diagnostic build (libsimaps_prof.so).

Loads the stamp build through SIMAPS_LIB, renders one batch (after a warm-up), and prints per-phase
wall time (median / max over workgroups, us) plus SSSP rounds.  Diagnostic only: the stamps
serialize nothing but add a few instructions; quote shares, not absolute kernel time."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ['SIMAPS_LIB'] = os.environ.get('SIMAPS_PROF_LIB', os.path.join(ROOT, 'spatial-intention-maps_amd', 'simaps', 'libsimaps_prof.so'))
sys.path.insert(0, os.path.join(ROOT, 'spatial-intention-maps_amd'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from simaps import _lib, batch, synthetic  # noqa: E402



def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='lifting_4-small_divider')
    ap.add_argument('--envs', type=int, default=64)
    ap.add_argument('--layout', default='chw')
    ap.add_argument('--dump', default=None, help='save the raw per-workgroup stamp table (.npy)')
    ap.add_argument('--alternate-maps', action='store_true',
                    help='flip one pixel of every slot\'s occupancy window before each render, so that the stamped render '
                         'is a state-cache miss (include/simaps_state_cache.h); the pixel, a window corner, changes no stack')
    args = ap.parse_args()
    L = _lib.lib
    L.simaps_debug_read_stamps.argtypes = [ctypes.c_void_p]
    scenes = [synthetic.make_scene(args.config, e) for e in range(args.envs)]
    b = batch.StateBatch(scenes, layout=args.layout)
    out = b.alloc_state()
    def flip():
        if args.alternate_maps:
            b.occupancy[:, b.cfg.room_i0 - 7, b.cfg.room_j0 - 7] ^= 1
    for _ in range(3):
        flip()
        b.render(out)
    torch.cuda.synchronize()
    # The stamp table lives on the device across launches: a slot that the stamped render did not write
    # still holds an earlier render's stamp (the warm-up's first render misses, so a hit would show the
    # miss path's stamps).  A time stamp that the render writes always changes, so one that is unchanged
    # since before the render counts as not recorded (0).  So does the round boundary's clock count
    # (stamp 79), which repeats in a workgroup by accident at most.  The counters may repeat: the SSSP
    # rounds (10) are written by every launch, and a wave's sweep steps (64 + w) count as recorded when
    # its sweep's end (24 + w) is.
    COUNTERS = [10] + list(range(64, 72))
    before = np.zeros((8192, 80), dtype=np.uint64)
    assert L.simaps_debug_read_stamps(before.ctypes.data) == 0
    st = np.zeros((8192, 80), dtype=np.uint64)
    flip()
    b.render(out)
    torch.cuda.synchronize()
    assert L.simaps_debug_read_stamps(st.ctypes.data) == 0
    stale = st == before
    stale[:, COUNTERS] = False
    st[stale] = 0
    for w in range(8):
        st[st[:, 24 + w] == 0, 64 + w] = 0
    st = st[:b.N].astype(np.int64)
    if args.dump:
        np.save(args.dump, st)
    def us(k1, k0):
        """median over workgroups of stamp k1 - stamp k0 (us); workgroups that recorded neither are
        left out, and a pair no workgroup recorded (a phase this build / config skips) is None."""
        m = (st[:, k1] > 0) & (st[:, k0] > 0)
        return float(np.median((st[m, k1] - st[m, k0]) / 100.0)) if m.any() else None
    def clk(k1, k0):
        """us() for two shader-clock stamps, in clocks"""
        m = (st[:, k1] > 0) & (st[:, k0] > 0)
        return float(np.median(st[m, k1] - st[m, k0])) if m.any() else None
    def clock_mhz():
        m = (st[:, 45] > 0) & (st[:, 44] > 0) & (st[:, 24] > st[:, 18]) & (st[:, 18] > 0)
        return float(np.median((st[m, 45] - st[m, 44]) / ((st[m, 24] - st[m, 18]) / 100.0))) if m.any() else None
    res = {'config': args.config, 'layout': args.layout, 'N': b.N,
           'total_us_median': us(6, 0), 'span_us': float((st[:, 6].max() - st[:, 0].min()) / 100.0),
           'sweep_track_us': {'agent_load': us(43, 0), 'first_ballot': us(46, 43), 'all_ballots': us(47, 46), 'v2_ballots_sync': us(15, 47), 'cspace_loads_ballots': us(15, 0), 'cspace_dilate': us(2, 15), 'cspace': us(2, 0), 'snap': us(48, 2), 'init': us(3, 48), 'rounds': us(49, 3), 'finish': us(50, 49), 'scale': us(7, 50), 'rounds_finish_scale': us(7, 3), 'end': us(7, 0)},
           'render_track_us': {'params': us(9, 0), 'blocksets': us(51, 9), 'stamp_tiles': us(1, 51), 'sampleidx_fast': us(40, 1), 'sampleidx_fp64': us(41, 40),
                               'gather_issue': us(42, 41), 'code_lookup': us(14, 42), 'overhead_robot': us(11, 14),
                               'raster_sync_wait': us(62, 11), 'raster_zero_sync': us(60, 62), 'raster_lines': us(61, 60), 'raster_endsync': us(13, 61), 'raster1': us(13, 11), 'sample_rest': us(8, 13), 'end': us(8, 0)},
           'params_us': {'rot_crop': us(72, 0), 'robot0': us(73, 0), 'seg_table0': us(74, 0), 'cmap_zero_w0': us(75, 0)},
           'join_us': us(4, 0),
           'distance_us': {'values': us(16, 5), 'block_min': us(17, 16), 'stores': us(6, 17), 'all': us(6, 5)},
           'sweep_rounds_us': {'round_%d' % r: us(19 + r, 18 + r) for r in range(3)},
           # (stamps 56 and 57 are the dilation's shader-clock stamps now, 63 and 78 are written nowhere)
           'check_r0_us': {'w0_sweep_end': us(24, 18), 'w3_sweep_end': us(27, 18)},
           'wave_sweep_r0_us': {'start': [us(32 + w, 18) for w in range(8)], 'end': [us(24 + w, 18) for w in range(8)]},
           'clock_mhz_sweep_w0': clock_mhz(),
           'dilate_clk_from52': {str(k): clk(k, 52) for k in (53, 54, 55, 56, 57, 58, 59) if clk(k, 52) is not None},
           'spread_us': {name: [float(np.percentile((st[:, k1].astype(np.int64) - st[:, 0].astype(np.int64)) / 100.0, q)) for q in (10, 50, 90, 100)]
                         for name, k1 in (('sweep_end', 7), ('render_end', 8), ('join', 4), ('total', 6))},
           'start_skew_us': float((np.percentile(st[:, 0], 100) - np.percentile(st[:, 0], 0)) / 100.0),
           'entry_skew_us': [float(np.percentile((st[:, 77] - st[:, 77].min()) / 100.0, q)) for q in (10, 50, 90, 100)],
           'entry_to_stamp0_us': [float(np.percentile((st[:, 0] - st[:, 77]) / 100.0, q)) for q in (10, 50, 90, 100)],
           # both tracks on the kernel-entry clock (stamp 77, the workgroup's own), so that builds whose stamp 0
           # sits elsewhere relative to the prologue's loads compare; render_start is the entry barrier (stamp
           # 0), which every wave leaves together
           'from_entry_us': {'render_start': us(0, 77), 'verdict': us(15, 77), 'rounds_start': us(3, 77),
                             'params_end': us(9, 77), 'sweep_end': us(7, 77), 'render_end': us(8, 77),
                             'join': us(4, 77), 'end': us(6, 77)},
           'end_after_first_entry_us': [float(np.percentile((st[:, 6] - st[:, 77].min()) / 100.0, q)) for q in (10, 50, 90, 100)],
           # stamp 79: source 0's round boundary between rounds 1 and 2 in shader clocks, the last
           # arriver's (ROUND_BOUNDARY_STAMP in csrc/simaps.hip); builds before it leave the slot 0
           'round_boundary_clk': ({'median': float(np.median(st[st[:, 79] > 0, 79])), 'p10': float(np.percentile(st[st[:, 79] > 0, 79], 10)),
                                   'p90': float(np.percentile(st[st[:, 79] > 0, 79], 90)), 'workgroups': int((st[:, 79] > 0).sum())}
                                  if (st[:, 79] > 0).any() else None),
           'sweep_steps_per_wave': [float(np.median(st[st[:, 24 + w] > 0, 64 + w])) if (st[:, 24 + w] > 0).any() else None
                                    for w in range(8)],
           'rounds': {'median': float(np.median(st[:, 10])), 'max': int(st[:, 10].max()), 'min': int(st[:, 10].min())}}
    # SSSP edge relaxations per stack -- every cell of a swept line evaluates its 3
    # incoming edges; wave w of source s sweeps direction (w + 2 s) & 3 (0 / 1: lines of w cells)
    h, w = b.cfg.room_h, b.cfg.room_w
    per_wave = [v or 0.0 for v in res['sweep_steps_per_wave']]
    res['sssp_relaxations_per_stack'] = float(sum(n * (w if ((k + 2 * (k >> 2)) & 3) < 2 else h) * 3
                                                  for k, n in enumerate(per_wave)))
    # drop the phases this build / config never stamped
    res = {k: ({q: v for q, v in d.items() if v is not None} if isinstance(d, dict) else d) for k, d in res.items()
           if d is not None}
    print(json.dumps(res, indent=1))


if __name__ == '__main__':
    main()
