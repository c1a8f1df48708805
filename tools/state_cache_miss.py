"""What a state-cache miss costs (include/simaps_state_cache.h): the flagship render timed with HIP events
while every slot's occupancy alternates between two map sets each step, so that every render misses
(each render finds the other set's window in its records and rewrites them).

    [SIMAPS_LIB=... SIMAPS_AB_SOURCE_HASH=...] python tools/state_cache_miss.py [--steps 200] [--warmup 20] [--tag NAME]
                                                                               [--family f32|into|bf16|f16]

--family: the launch that is timed -- the float32 render (default, as before), render_into of a bf16
store of 4,096 rows (simaps_get_state_into_cached), or the bf16 / fp16 render (simaps_get_state_as_cached).

One JSON line: the median / min / max per-render time in us and the records' counters.  A library
without the cached entry point (another revision's build, for the A/B) renders through
simaps_get_state, which is what a miss is compared with.  The map copy lies between the timed regions.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'spatial-intention-maps_amd'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from simaps import _lib, batch, synthetic  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='lifting_4-small_divider')
    ap.add_argument('--envs', type=int, default=64)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--family', default='f32', choices=['f32', 'into', 'bf16', 'f16'])
    ap.add_argument('--tag', default=os.environ.get('SIMAPS_LIB', 'product'))
    args = ap.parse_args()
    scenes = [synthetic.make_scene(args.config, e) for e in range(args.envs)]
    # (the store and 16-bit launches pass the cache only on request: state_cache='all')
    b = batch.StateBatch(scenes, state_cache=True if args.family == 'f32' else 'all')
    other = [synthetic.make_scene(args.config, args.envs + e) for e in range(args.envs)]
    sets = [b.occupancy.clone(),
            torch.from_numpy(np.stack([other[e]['occupancy'][a] for e, a in b.agents]).astype(np.uint8)).to(b.device)]
    i0, j0, h, w = b.cfg.room_i0, b.cfg.room_j0, b.cfg.room_h, b.cfg.room_w
    win = (slice(None), slice(i0 - 7, i0 + h + 7), slice(j0 - 7, j0 + w + 7))
    sets[1][:, i0 - 7, j0 - 7] = 1 - sets[0][:, i0 - 7, j0 - 7].clamp(max=1)  # (a window corner: beyond every dilation's reach)
    differ = (sets[0][win] != sets[1][win]).flatten(1).any(1)
    assert bool(differ.all()), 'every slot needs two different windows'
    if args.family == 'into':
        store = b.alloc_store(4096, torch.bfloat16)
        dest = torch.from_numpy(np.random.RandomState(7).permutation(4096)[:b.N].astype(np.int64)).to(b.device)
        launch = lambda: b.render_into(store, dest)  # noqa: E731
    else:
        out = b.alloc_state(dtype={'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}[args.family])
        launch = lambda: b.render(out)  # noqa: E731
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
    for k in range(args.warmup + args.steps):
        b.occupancy.copy_(sets[k & 1])
        if k >= args.warmup:
            evs[k - args.warmup][0].record()
        launch()
        if k >= args.warmup:
            evs[k - args.warmup][1].record()
    torch.cuda.synchronize()
    _lib.check_faults()
    us = np.array([a.elapsed_time(z) * 1e3 for a, z in evs])
    hd = b.state_cache_headers()
    res = {'tool': 'state_cache_miss', 'build': args.tag, 'family': args.family, 'config': args.config, 'stacks': b.N, 'steps': args.steps,
           'median_us': float(np.median(us)), 'min_us': float(us.min()), 'max_us': float(us.max()),
           'p10_us': float(np.percentile(us, 10)), 'p90_us': float(np.percentile(us, 90)),
           'cached_entry': hd is not None,
           'hits': None if hd is None else int(hd['hits'].sum()), 'misses': None if hd is None else int(hd['misses'].sum())}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
