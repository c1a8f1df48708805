"""Host-side profiles of the drop-in observation step (VectorEnvObservations) on the GPU box.  Diagnostic only.

    python tools/dropin_profile.py            cProfile of update + get_state: where the host time of a step goes
    python tools/dropin_profile.py --remap    deferred against immediate periodic re-maps (RobotController.step,
                                              envs.py:1401-1403), written to profiles/ingest_seq_dropin.jsonl:
        row A  K immediate update_map calls, each after its update_arrays, then one synchronize
        row B  K queue_map_update calls, each after its update_arrays, one flush_map_updates, then one synchronize
      for K = 16 frames of one robot and K = 64 frames over 16 robots; the frames are host arrays, as
      getCameraImage returns them.  A and B alternate five times in one process; median and min-max.
"""
import argparse
import cProfile
import json
import os
import pstats
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'spatial-intention-maps_amd'))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from simaps import batch, synthetic, vector_env  # noqa: E402


def profile_step():
    scenes = [synthetic.make_scene('lifting_4-small_divider', e) for e in range(64)]
    obs = vector_env.VectorEnvObservations(scenes, layout='chw')

    def step():
        obs.update(scenes=scenes)
        obs.get_state()
        torch.cuda.synchronize()

    for _ in range(10):
        step()
    pr = cProfile.Profile()
    pr.enable()
    for _ in range(100):
        step()
    pr.disable()
    pstats.Stats(pr).sort_stats('tottime').print_stats(18)


def profile_remap(out, rounds=5):
    config, envs = 'lifting_4-small_divider', 16
    scenes = [synthetic.make_scene(config, e) for e in range(envs)]
    obs = vector_env.VectorEnvObservations(scenes, layout='chw')
    arrays = batch.descriptor_arrays(scenes)
    frames = [synthetic.camera_images(scenes[e], 2, 'forward', seed=e) for e in range(4)]
    frames = [(d[None], s[None].astype(np.int32)) for d, s in frames]
    rows = []
    for name, robots in (('16_frames_1_robot', [(3, 2)] * 16),
                         ('64_frames_16_robots', [(e, 2) for e in range(16)] * 4)):
        K = len(robots)

        def immediate():
            for k, ea in enumerate(robots):
                obs.update_arrays(**arrays)
                obs.update_map([ea], *frames[k % 4])
            torch.cuda.synchronize()

        def deferred():
            for k, ea in enumerate(robots):
                obs.update_arrays(**arrays)
                obs.queue_map_update([ea], *frames[k % 4])
            obs.flush_map_updates()
            torch.cuda.synchronize()

        ts = {'immediate': [], 'deferred': []}
        for fn in (immediate, deferred):  # warm-up: allocations, the staging buffer
            fn(), fn()
        for _ in range(rounds):
            for key, fn in (('immediate', immediate), ('deferred', deferred)):
                t0 = time.perf_counter()
                fn()
                ts[key].append((time.perf_counter() - t0) * 1e3)
        for row, key in (('A_immediate', 'immediate'), ('B_deferred', 'deferred')):
            t = ts[key]
            rows.append({'row': row, 'case': name, 'config': config, 'frames': K, 'rounds': rounds,
                         'ms_median': float(np.median(t)), 'ms_min': min(t), 'ms_max': max(t),
                         'ms_per_frame_median': float(np.median(t)) / K})
    rows.append({'row': 'note', 'note': 'end to end including the final synchronize; host (pageable NumPy) frames; every '
                 'frame after its own update_arrays; A and B alternate round by round in one process; read against '
                 'remap_one_robot (profiles/archive/r3p_dropin_bench.jsonl: 0.080 ms, frame already on the device, no '
                 'update_arrays)'})
    text = ''.join(json.dumps(r) + '\n' for r in rows)
    print(text, end='', flush=True)
    with open(out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--remap', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ingest_seq_dropin.jsonl'))
    args = ap.parse_args()
    if args.remap:
        profile_remap(args.out)
    else:
        profile_step()
