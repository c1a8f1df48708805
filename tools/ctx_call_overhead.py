"""Host cost of a context twin against the old entry point (GPU box): simaps_ctx_get_state through a
created context against simaps_get_state, at N = 1, in alternating legs of back-to-back launches with
one synchronize per leg.  Per leg: host microseconds per call to issue the launches, and wall
microseconds per call including the final synchronize (at N = 1 the kernel outlasts the call, so
once the queue is full the host figure follows the kernel).  A second pair of legs calls both with
N = 0, which returns after the argument checks and launches nothing: the twin's own cost -- the
registry lookup and the device check -- with no GPU time in it.  This measures overhead on purpose;
a reported number, not a gate.  One JSON line per leg and a summary line.

    python tools/ctx_call_overhead.py [--calls 3000] [--rounds 5] [--out profiles/ctx_call_overhead.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'spatial-intention-maps_amd'))
import torch  # noqa: E402

from simaps import _lib, batch, context, synthetic  # noqa: E402


def leg(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return (t1 - t0) / n * 1e6, (t2 - t0) / n * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=3000)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ctx_call_overhead.jsonl'))
    a = ap.parse_args()
    b = batch.StateBatch([synthetic.make_scene('lifting_4-small_divider', 0)], agents=[(0, 0)])
    assert b.N == 1
    out = b.alloc_state()
    s = torch.cuda.current_stream()
    L = _lib.lib
    ctx = context.Context()

    def args(n):
        return (b.cfg, n, _lib.ptr(b.agents_d), _lib.ptr(b.envs_d), _lib.ptr(b.robots_d), _lib.ptr(b.paths_d),
                _lib.ptr(b.occupancy), _lib.ptr(b.overhead), _lib.ptr(out), 0, None, _lib.stream_handle(s))

    legs = []
    for what, n in (('launch_n1', 1), ('checks_only_n0', 0)):
        ar = args(n)
        fns = {'old': lambda: L.simaps_get_state(*ar), 'twin': lambda: L.simaps_ctx_get_state(ctx.handle, *ar)}
        for name in fns:  # warm-up, and the calls must succeed
            for _ in range(50):
                assert fns[name]() == 0, L.simaps_last_error()
        for r in range(a.rounds):
            for name in ('old', 'twin'):
                host, wall = leg(fns[name], a.calls)
                legs.append({'what': what, 'entry': name, 'round': r, 'calls': a.calls, 'host_us_per_call': round(host, 3),
                             'wall_us_per_call': round(wall, 3)})
    assert ctx.fault_status() == 0 and L.simaps_fault_status(0) == 0
    ctx.close()
    summary = {'summary': True, 'device': torch.cuda.get_device_name(0)}
    for what in ('launch_n1', 'checks_only_n0'):
        for name in ('old', 'twin'):
            for key in ('host_us_per_call', 'wall_us_per_call'):
                v = [x[key] for x in legs if x['what'] == what and x['entry'] == name]
                summary['%s_%s_%s' % (what, name, key)] = {'median': round(statistics.median(v), 3), 'min': min(v),
                                                           'max': max(v)}
    with open(a.out, 'w') as f:
        for x in legs + [summary]:
            f.write(json.dumps(x) + '\n')
    print(json.dumps(summary))


if __name__ == '__main__':
    main()
