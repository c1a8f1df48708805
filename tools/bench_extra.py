"""Throughput of the SURVEY.md 8(f) rows built so far, GPU vs the CPU oracle (1 core):

  sp_distance    OccupancyMap.shortest_path_distance (reward lookups): queries/s
  shortest_path  OccupancyMap.shortest_path (movement paths): paths/s
  ingest         Robot.update_map minus the simulator (camera frame -> overhead / occupancy maps): frames/s
  distance_to_receptacle  the reward lookups from the receptacle, cold and from the render's cache
  env_step       (--env-step) the device time of one reference VectorEnv.step: paths, ingest, get_state
  mixed          (--mixed) one launch over envs of the BASELINE configurations together
                 (simaps_get_state_mixed) vs one launch per configuration back to back
  store_new_action (--action) the step back from the policy (simaps_store_new_action): device time
                 of the call and of its decode kernel, and the wall time per step against the same
                 result composed from torch arg-max + numpy + shortest_paths + set_descriptor_arrays
                 then (also alone: --action-as) simaps_store_new_action_as: bf16 Q maps through it
                 against a .float() cast + the old call, float32 through it against the old call, and
                 the device exploration draw; rounds alternating, all recorded
  state16        (--state16) the state stack rendered directly as bf16 / fp16 (simaps_get_state_as)
                 against the float32 render and the float32 render + cast pass: device time per
                 256 stacks, the four alternating in one process
  store          (--store) states rendered straight into a bf16 store of 4,096 stacks at rows chosen
                 by a device-side dest (simaps_get_state_into) against today's route, the render into
                 a ring batch + index_copy_ into the store: all 256 agents, and a 64-agent subset
  gridgraph_large (--gridgraph-large) GridGraph on a 500 x 500 grid (beyond the LDS window: the
                 global-memory kernels of csrc/grid_large.h): images and paths, 1 and 64 per call

    python tools/bench_extra.py [--config lifting_4-small_divider] [--envs 64] [--queries 8]

Prints one JSON line per row.  Inputs resident in HBM; timing with torch.cuda events around K
launches after warm-up.  The CPU leg times the oracle (the checker) on a bounded sample.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'spatial-intention-maps_amd'))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from simaps import batch, synthetic  # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='lifting_4-small_divider')
    ap.add_argument('--envs', type=int, default=64)
    ap.add_argument('--queries', type=int, default=8, help='reward-lookup targets per agent')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--cpu-budget', type=float, default=8.0)
    args = ap.parse_args()
    import oracle
    scenes = [synthetic.make_scene(args.config, e) for e in range(args.envs)]
    b = batch.StateBatch(scenes)
    rs = np.random.RandomState(0)
    s0 = scenes[0]
    rl, rw = s0['room_length'], s0['room_width']
    N, Q = b.N, args.queries
    rec = s0['receptacle_position']
    src = np.array([rec[:2] if rec is not None else scenes[e]['robots'][a]['position'][:2] for e, a in b.agents])
    tgt = np.stack([rs.uniform(-rl / 2, rl / 2, (N, Q)), rs.uniform(-rw / 2, rw / 2, (N, Q))], -1)
    src_d = torch.as_tensor(src).cuda()
    tgt_d = torch.as_tensor(tgt).cuda()
    dt = timed(lambda: b.shortest_path_distances(src_d, tgt_d), args.steps, 3)
    # CPU oracle on a bounded sample
    n, el = 0, 0.0
    for (e, a) in b.agents:
        t0 = time.perf_counter()
        ao = oracle.AgentOracle(scenes[e], a)
        k = b.agents.index((e, a))
        for q in range(Q):
            ao.shortest_path_distance(src[k], tgt[k, q])
        el += time.perf_counter() - t0
        n += Q
        if el > args.cpu_budget:
            break
    print(json.dumps({'row': 'sp_distance', 'config': args.config, 'agents': N, 'queries_per_agent': Q,
                      'gpu_queries_per_s': N * Q / dt, 'gpu_ms_per_launch': dt * 1e3,
                      'cpu_oracle_queries_per_s': n / el, 'cpu_cores': 1,
                      'cpu_sample': '%d queries incl. each agent\'s cspace / EDT / SPFA' % n}), flush=True)
    if rec is not None:
        # reward lookups from the receptacle (Mapper.distance_to_receptacle): cold = the full SSSP per
        # call (no cache); cached = the arrays the last render left (simaps_sp_lookup), as the
        # reference's GridGraph cache answers between two map updates
        cold = timed(lambda: b.receptacle_distances(tgt_d, cache=False), args.steps, 3)
        b.enable_receptacle_cache()
        b.render()
        cached = timed(lambda: b.receptacle_distances(tgt_d), args.steps, 3)
        assert (b._rec_ver == b._map_ver).all()
        got_c = b.receptacle_distances(tgt_d).cpu().numpy()
        got_f = b.receptacle_distances(tgt_d, cache=False).cpu().numpy()
        print(json.dumps({'row': 'distance_to_receptacle', 'config': args.config, 'agents': N, 'queries_per_agent': Q,
                          'cold_ms_per_call': cold * 1e3, 'cached_ms_per_call': cached * 1e3,
                          'cold_queries_per_s': N * Q / cold, 'cached_queries_per_s': N * Q / cached,
                          'cached_equals_cold': bool(np.array_equal(got_c, got_f)),
                          'note': 'StateBatch.receptacle_distances per call incl. host side; cached: every slot '
                                  'rendered since its last map change (simaps_sp_lookup), cold: cache=False '
                                  '(cspace + snap + SSSP per agent, simaps_sp_distance)'}), flush=True)

    # movement paths: robot position -> random target (half across x = 0)
    psrc = np.array([scenes[e]['robots'][a]['position'][:2] for e, a in b.agents])
    ptgt = np.stack([rs.uniform(0.05, rl / 2, N) * -np.sign(psrc[:, 0]), rs.uniform(-rw / 2, rw / 2, N)], -1)
    dt = timed(lambda: b.shortest_paths(psrc, ptgt), max(3, args.steps // 4), 1)
    n, el = 0, 0.0
    for k, (e, a) in enumerate(b.agents):
        t0 = time.perf_counter()
        oracle.AgentOracle(scenes[e], a).shortest_path(psrc[k], ptgt[k])
        el += time.perf_counter() - t0
        n += 1
        if el > args.cpu_budget:
            break
    print(json.dumps({'row': 'shortest_path', 'config': args.config, 'paths_per_launch': N,
                      'gpu_paths_per_s': N / dt, 'gpu_ms_per_launch_incl_d2h': dt * 1e3,
                      'cpu_oracle_paths_per_s': n / el, 'cpu_cores': 1,
                      'cpu_sample': '%d paths incl. each agent\'s cspace / EDT / SPFA' % n}), flush=True)


def bench_dropin_step(args):
    """The drop-in's host + device cost of one observation step: VectorEnvObservations.update(new
    scene descriptors) + get_state() (device tensors, every robot), synchronised -- what a training
    loop pays per step beside its simulator (the bench line times the kernel alone)."""
    from simaps import vector_env
    scenes = [synthetic.make_scene(args.config, e) for e in range(args.envs)]
    arrays = batch.descriptor_arrays(scenes)
    n = sum(len(s['robots']) for s in scenes)
    for mode in ('scenes', 'arrays', 'arrays+ring'):
        obs = vector_env.VectorEnvObservations(scenes, layout='chw', reuse_outputs=2 if mode == 'arrays+ring' else 0)
        if mode == 'scenes':
            upd = lambda: obs.update(scenes=scenes)  # noqa: E731
        else:
            upd = lambda: obs.update_arrays(**arrays)  # noqa: E731

        def step():
            upd()
            obs.get_state()
            torch.cuda.synchronize()
        for _ in range(5):
            step()
        ts, tu, tg = [], [], []
        for _ in range(max(args.steps, 300)):  # per-step times: the median resists the shared host's noise
            t0 = time.perf_counter()
            upd()
            t1 = time.perf_counter()
            obs.get_state()
            t2 = time.perf_counter()
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            ts.append(t3 - t0)
            tu.append(t1 - t0)
            tg.append(t2 - t1)
        dt = float(np.median(ts))
        print(json.dumps({'row': 'dropin_step', 'update': mode, 'config': args.config, 'stacks_per_step': n,
                          'ms_per_step': dt * 1e3, 'ms_per_step_mean': float(np.mean(ts)) * 1e3,
                          'host_update_ms': float(np.median(tu)) * 1e3, 'host_get_state_ms': float(np.median(tg)) * 1e3,
                          'stacks_per_s_end_to_end': n / dt,
                          'note': 'update(%s) + get_state() + synchronize, host packing and uploads included; '
                                  'median of %d steps' % (mode, len(ts))}),
              flush=True)


def bench_env_step(args):
    """the device work of one reference VectorEnv.step (envs.py:230-320) at
    BASELINE configs[1] (64 envs x 4 lifting robots), for E awaiting robots (default one per env, the
    steady state; --all: every robot, the first step): movement paths for the new actions
    (store_new_action -> Mapper.shortest_path, envs.py:234 -> 875-876; targets in the robot's local
    map, the action space), the awaiting robots' update_map (envs.py:277-280: a forward camera frame
    each) and their get_state render (envs.py:304, 322-323).  Each launch's device time by HIP
    events (K back-to-back launches of that part alone) and the three together, in step order, one
    stream.  Run it under rocprofv3 --kernel-trace --stats for the per-kernel split."""
    scenes = [synthetic.make_scene(args.config, e) for e in range(args.envs)]
    b = batch.StateBatch(scenes)
    A = len(scenes[0]['robots'])
    slots = list(range(b.N)) if args.all else [e * A + (e % A) for e in range(args.envs)]
    n = len(slots)
    rs = np.random.RandomState(4)
    psrc = np.array([scenes[e]['robots'][a]['position'][:2] for e, a in (b.agents[k] for k in slots)])
    ptgt = psrc + rs.uniform(-0.5, 0.5, psrc.shape)   # inside the robot's local map
    src_d, tgt_d = torch.as_tensor(psrc).cuda(), torch.as_tensor(ptgt).cuda()
    frames = [synthetic.camera_images(scenes[e], a, 'forward', seed=k) for k, (e, a) in enumerate(b.agents[k] for k in slots)]
    dep = torch.as_tensor(np.stack([f[0] for f in frames])).cuda()
    seg = torch.as_tensor(np.stack([f[1] for f in frames]).astype(np.int32)).cuda()
    prep = b.prepare_ingest(dep, seg, camera='forward', slots=slots)
    out = b.alloc_state(n)
    s = torch.cuda.current_stream()
    parts = {'paths': lambda: b.launch_shortest_paths(src_d, tgt_d, slots=slots),
             'ingest': lambda: b.launch_ingest(prep),
             'get_state': lambda: b.render(out, slots=slots)}
    parts['step'] = lambda: [f() for f in (parts['paths'], parts['ingest'], parts['get_state'])]
    res = {}
    K = max(args.steps, 20)
    for name, f in parts.items():
        for _ in range(3):
            f()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(K):
            f()
        e1.record(s)
        torch.cuda.synchronize()
        res[name + '_us'] = e0.elapsed_time(e1) / K * 1e3
    print(json.dumps(dict({'row': 'env_step', 'config': args.config, 'awaiting_robots': n,
                           'note': 'device time per reference step (HIP events, %d launches each): movement paths '
                                   '(automatic path mode: the overlapped early-exit kernel at this size, local-map targets), forward-camera ingest, get_state of the '
                                   'awaiting robots; step = the three in order on one stream' % K}, **res)),
          flush=True)


def _host_store_new_action(b, q, slots, arr, rob_idx, ee_offset, P):
    """The new call's result composed from what the library offered before it: torch arg-max +
    .tolist(), numpy geometry, the movement-path launch + download, numpy post-processing (vectorised
    over the robots), set_descriptor_arrays.  Robot.store_new_action, envs.py:857-903."""
    n = len(slots)
    a = np.asarray(q.view(n, -1).argmax(1).tolist())
    rem = a % 9216
    row, col = rem // 96, rem % 96
    dx, dy = ((col + 0.5) - 48.0) / 96.0, (48.0 - (row + 0.5)) / 96.0
    pos, heading = arr['pose'][rob_idx, :2], arr['pose'][rob_idx, 2]
    dist = np.sqrt(dx * dx + dy * dy)
    theta = heading + np.arctan2(-dx, dy)
    tgt = pos + dist[:, None] * np.stack([np.cos(theta), np.sin(theta)], 1)
    xy, cnt = b.launch_shortest_paths(pos, tgt, slots=slots, max_points=P)
    xy, cnt = xy.cpu().numpy(), cnt.cpu().numpy()
    rh = lambda h: (h + np.pi) % (2 * np.pi) - np.pi  # noqa: E731
    d = xy[:, 1:] - xy[:, :-1]
    hd = np.concatenate([heading[:, None], rh(np.arctan2(d[..., 1], d[..., 0]))], 1)
    k = np.arange(n)
    last = cnt - 1
    e = xy[k, last] - xy[k, last - 1]
    sd = np.sqrt(e[:, 0] ** 2 + e[:, 1] ** 2) - ee_offset
    hl = hd[k, last]
    xy[k, last] = xy[k, last - 1] + sd[:, None] * np.stack([np.cos(hl), np.sin(hl)], 1)
    fix = np.nonzero((cnt > 2) & (sd < 0))[0]
    if len(fix):
        lf = last[fix]
        xy[fix, lf - 1] = xy[fix, lf]
        e = xy[fix, lf - 1] - xy[fix, lf - 2]
        hd[fix, lf - 1] = rh(np.arctan2(e[:, 1], e[:, 0]))
    arr['target'][rob_idx] = tgt
    arr['idle'][rob_idx] = False
    arr['waypoints'][rob_idx] = xy
    arr['wp_count'][rob_idx] = cnt
    arr['wp_index'][rob_idx] = 1
    b.set_descriptor_arrays(**arr)
    return a, tgt, xy, hd, cnt


def bench_action(args):
    """The step back from the policy (include/simaps_action.h) for `awaiting` robots of 64 envs of
    lifting_4-small_divider, Q maps resident on the device as the networks leave them:
    (a) device time by HIP events after warm-up: the whole call (decode, path, finish; write-back on),
        and the decode kernel: the call without the path launch, with the Q maps read minus with every
        action given (the same two launches, the decode workgroups then skip their Q block) -- the
        difference is the Q read, reported with its bytes per second;
    (b) wall time per step, synchronised, results downloaded to the host in both routes: the new call
        (store_new_actions(write_back=True) + one download) against _host_store_new_action; the two
        alternate step by step in this process; medians."""
    from simaps import _lib, constants as K
    scenes = [synthetic.make_scene(args.config, e) for e in range(args.envs)]
    A = len(scenes[0]['robots'])
    P = _lib.MAX_PATH
    lines = []
    for n in args.awaiting:
        b = batch.StateBatch(scenes)
        slots = list(range(b.N)) if n == b.N else [e * A + (e % A) for e in range(args.envs)][:n]
        assert len(slots) == n
        rob_idx = np.asarray(slots)  # (every agent in order: slot k is robot k)
        arr = batch.descriptor_arrays(scenes)
        w = np.zeros((b.n_robots, P, 2))
        w[:, :arr['waypoints'].shape[1]] = arr['waypoints']
        arr['waypoints'] = w
        b.set_descriptor_arrays(**arr)
        q = torch.randn(n, 2, 96, 96, generator=torch.Generator().manual_seed(1)).cuda()
        given = torch.as_tensor(q.view(n, -1).argmax(1), dtype=torch.int32)
        ee = K.ROBOT_GEOM['lifting_robot']['END_EFFECTOR_LOCATION'] + K.CUBE_WIDTH / 2  # envs.py:889
        s = torch.cuda.current_stream()
        qf, q_off = q.view(-1), torch.arange(n, dtype=torch.int64, device='cuda') * (2 * 9216)
        parts = {'call': lambda: b.store_new_actions(q=qf, q_off=q_off, slots=slots, max_points=P, write_back=True),
                 'paths_alone': lambda: b.launch_shortest_paths(src_d, tgt_d, slots=slots, max_points=P),
                 'decode_finish': lambda: b.store_new_actions(q=qf, q_off=q_off, slots=slots, max_points=P,
                                                              use_shortest_path_movement=False),
                 'finish_given': lambda: b.store_new_actions(q=qf, q_off=q_off, actions=given, slots=slots, max_points=P,
                                                             use_shortest_path_movement=False)}
        big = torch.randn(8192, 8192, device='cuda')
        r0 = parts['call']()
        src_d, tgt_d = r0.source.clone(), r0.target.clone()
        res = {}
        reps = max(args.steps, 50)
        for name, f in parts.items():
            for _ in range(5):
                f()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            # a few ms of other work first: the calls below queue up behind it and then run back to
            # back, so the events see the device time and not the host's ~30 us per Python call
            torch.mm(big, big)
            e0.record(s)
            for _ in range(reps):
                f()
            e1.record(s)
            torch.cuda.synchronize()
            res[name + '_us'] = e0.elapsed_time(e1) / reps * 1e3
        nbytes = n * 2 * 9216 * 4
        dec = res['decode_finish_us'] - res['finish_given_us']
        lines.append(dict({'row': 'store_new_action_device', 'config': args.config, 'awaiting_robots': n,
                           'q_bytes': nbytes, 'decode_us': dec, 'decode_GBps': nbytes / max(dec, 1e-3) / 1e3,
                           'decode_share_of_call': dec / res['call_us'],
                           'note': 'HIP events around %d calls queued behind a blocking kernel (device-bound) after warm-up; '
                                   'decode_finish / finish_given: the call without the path launch, Q maps read / every '
                                   'action given (the decode workgroups skip the read); decode_us is their difference'
                                   % reps}, **res))
        print(json.dumps(lines[-1]), flush=True)

        def new_route():
            h = b.store_new_actions(q=q, slots=slots, max_points=P, write_back=True).to_host()
            torch.cuda.synchronize()
            return h

        def new_route_device_only():
            b.store_new_actions(q=q, slots=slots, max_points=P, write_back=True)
            torch.cuda.synchronize()

        def old_route():
            r = _host_store_new_action(b, q, slots, arr, rob_idx, ee, P)
            torch.cuda.synchronize()
            return r
        for _ in range(5):
            new_route(), old_route(), new_route_device_only()
        h, o = new_route(), old_route()
        assert np.array_equal(h['action'], o[0]) and np.array_equal(h['count'], o[4])  # the same result
        tn, to, td = [], [], []
        for _ in range(max(args.steps, 200)):
            for f, acc in ((new_route, tn), (old_route, to), (new_route_device_only, td)):
                t0 = time.perf_counter()
                f()
                acc.append(time.perf_counter() - t0)
        mn, mo, md = (float(np.median(t)) * 1e3 for t in (tn, to, td))
        lines.append({'row': 'store_new_action_step', 'config': args.config, 'awaiting_robots': n,
                      'new_ms': mn, 'composed_ms': mo, 'speedup': mo / mn, 'new_without_download_ms': md,
                      'note': 'wall time per step, synchronised, medians of %d alternating steps: new = '
                              'store_new_actions(write_back) + download of the results; composed = torch arg-max + '
                              '.tolist(), numpy geometry, launch_shortest_paths + download, vectorised numpy '
                              'post-processing, set_descriptor_arrays' % len(tn)})
        print(json.dumps(lines[-1]), flush=True)
    out = os.path.join(ROOT, 'profiles', 'action_bench.jsonl')
    with open(out, 'w') as f:
        f.write(''.join(json.dumps(x) + '\n' for x in lines))


def bench_action_as(args):
    """simaps_store_new_action_as (include/simaps_action_as.h) against the routes it replaces, for
    `awaiting` robots of 64 envs of lifting_4-small_divider: the call without the path launch (decode +
    finish: the part that reads the Q maps), by bench_action's method -- HIP events around `reps` calls
    queued behind a blocking kernel -- with the variants alternating round by round in this process.
    Variants: f32_old (simaps_store_new_action), f32_as (the same input through the new entry point),
    bf16_as (bf16 Q maps through the new entry point), cast_f32_old (the route bf16 outputs take
    without it: a .float() pass, then the old call), bf16_as_eps (bf16_as with the device draw at
    eps 0.1 and the kernel that advances the rng state).  Every round of every variant is recorded;
    f32_as_within_f32_old says whether every f32_as round lies inside min..max of the f32_old rounds."""
    from simaps import _lib, policy_output
    scenes = [synthetic.make_scene(args.config, e) for e in range(args.envs)]
    A = len(scenes[0]['robots'])
    P = 2
    lines = []
    big = torch.randn(8192, 8192, device='cuda')
    s = torch.cuda.current_stream()
    for n in args.awaiting:
        b = batch.StateBatch(scenes)
        slots = list(range(b.N)) if n == b.N else [e * A + (e % A) for e in range(args.envs)][:n]
        agents_d, _ = b.subset_descriptor(slots)
        q32 = torch.randn(n, 2, 96, 96, generator=torch.Generator().manual_seed(1)).cuda().view(-1)
        q16 = q32.to(torch.bfloat16)
        q_off = torch.arange(n, dtype=torch.int64, device='cuda') * (2 * 9216)
        eps = torch.full((n,), 0.1, dtype=torch.float32, device='cuda')
        rng = policy_output.DeviceExploration(1, 'cuda')
        i32 = lambda *sh: torch.empty(sh, dtype=torch.int32, device='cuda')  # noqa: E731
        f64 = lambda *sh: torch.empty(sh, dtype=torch.float64, device='cuda')  # noqa: E731
        outs = [i32(n), f64(n, 2), f64(n, 2), f64(n, P, 2), f64(n, P), i32(n)]
        explored = torch.empty(n, dtype=torch.uint8, device='cuda')
        head = [b.cfg, n, _lib.ptr(agents_d), _lib.ptr(b.envs_d), _lib.ptr(b.robots_d), _lib.ptr(b.paths_d),
                _lib.ptr(b.occupancy)]
        tail = [0, P] + [_lib.ptr(t) for t in outs]
        sh = _lib.stream_handle(s)

        def old(q):
            _lib.check(_lib.lib.simaps_store_new_action(*(head + [_lib.ptr(q), _lib.ptr(q_off), None] + tail + [sh])))

        def new(q, dt, e=None, r=None, x=None):
            _lib.check(_lib.lib.simaps_store_new_action_as(*(head + [_lib.ptr(q), dt, _lib.ptr(q_off), None, _lib.ptr(e),
                                                                     _lib.ptr(r)] + tail + [_lib.ptr(x), sh])))
        variants = {'f32_old': lambda: old(q32),
                    'f32_as': lambda: new(q32, _lib.STATE_F32),
                    'bf16_as': lambda: new(q16, _lib.STATE_BF16),
                    'cast_f32_old': lambda: old(q16.float()),
                    'bf16_as_eps': lambda: new(q16, _lib.STATE_BF16, eps, rng.tensor, explored)}
        for f in variants.values():
            for _ in range(5):
                f()
        torch.cuda.synchronize()
        runs = {k: [] for k in variants}
        for _ in range(args.rounds):
            for name, f in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.mm(big, big)  # (the calls below queue up behind it and then run back to back)
                e0.record(s)
                for _ in range(args.reps):
                    f()
                e1.record(s)
                torch.cuda.synchronize()
                runs[name].append(e0.elapsed_time(e1) / args.reps * 1e3)
        lo, hi = min(runs['f32_old']), max(runs['f32_old'])
        lines.append({'row': 'store_new_action_as_device', 'config': args.config, 'awaiting_robots': n,
                      'median_us': {k: float(np.median(v)) for k, v in runs.items()},
                      'runs_us': {k: [round(x, 3) for x in v] for k, v in runs.items()},
                      'f32_as_within_f32_old': bool(all(lo <= x <= hi for x in runs['f32_as'])),
                      'note': 'decode + finish (no path launch, max_points 2), direct ABI calls into preallocated outputs; '
                              'HIP events around %d calls queued behind a blocking kernel, %d rounds, the variants '
                              'alternating round by round' % (args.reps, args.rounds)})
        print(json.dumps(lines[-1]), flush=True)
    out = os.path.join(ROOT, 'profiles', 'action_as_bench.jsonl')
    with open(out, 'w') as f:
        f.write(''.join(json.dumps(x) + '\n' for x in lines))


def bench_state16(args):
    """The render launch of `envs` envs of `config` (BASELINE configs[1]: 256 stacks), CHW, as
    (a) float32, (b) float32 + the cast pass a 16-bit consumer needs today (copy_ into a preallocated
    bfloat16 batch), (c) bfloat16 and (d) float16 written by the fused kernel.  Device time by HIP
    events around `reps` calls queued behind a blocking kernel (so the events see the device and not
    the host's per-call time); the four variants alternate round by round in this process, and each
    reports its rounds' median, min and max.  (c) and (d) do (a)'s work with fewer bytes written, so
    they are expected within (a)'s own min..max of this session or below; (b) - (c) is the gain."""
    scenes = [synthetic.make_scene(args.config, e) for e in range(args.envs)]
    # --state-cache: the 16-bit renders pass the batch's state cache too (off by default: DESIGN.md section 5)
    b = batch.StateBatch(scenes, layout='chw', state_cache='all' if args.state_cache else True)
    f32 = b.alloc_state()
    o16 = {dt: b.alloc_state(dtype=dt) for dt in (torch.bfloat16, torch.float16)}
    cast = b.alloc_state(dtype=torch.bfloat16)

    def render_and_cast():
        b.render(out=f32)
        cast.copy_(f32)
    variants = {'a_f32': lambda: b.render(out=f32), 'b_f32_plus_cast_bf16': render_and_cast,
                'c_bf16': lambda: b.render(out=o16[torch.bfloat16]), 'd_f16': lambda: b.render(out=o16[torch.float16])}
    for f in variants.values():
        for _ in range(20):
            f()
    torch.cuda.synchronize()
    assert torch.equal(o16[torch.bfloat16], cast) and torch.equal(o16[torch.float16], f32.to(torch.float16))
    big = torch.randn(8192, 8192, device='cuda')
    s = torch.cuda.current_stream()
    us = {k: [] for k in variants}
    for _ in range(args.rounds):
        for name, f in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.mm(big, big)
            torch.mm(big, big)
            e0.record(s)
            for _ in range(args.reps):
                f()
            e1.record(s)
            torch.cuda.synchronize()
            us[name].append(e0.elapsed_time(e1) / args.reps * 1e3)
    from simaps import _lib
    _lib.check_faults()
    a_lo, a_hi = min(us['a_f32']), max(us['a_f32'])
    elems = b.N * b.C * 96 * 96
    lines = []
    for name, v in us.items():
        line = {'row': 'state16', 'variant': name, 'config': args.config, 'stacks': b.N, 'channels': b.C, 'layout': 'chw',
                'median_us': float(np.median(v)), 'min_us': min(v), 'max_us': max(v), 'rounds_us': [round(x, 3) for x in v],
                'state_bytes_written': elems * (4 if name.startswith(('a_', 'b_')) else 2),
                'cast_pass_bytes': elems * 6 if name.startswith('b_') else 0, 'reps_per_round': args.reps,
                'state_cache': 'all' if args.state_cache else 'float32 render only'}
        if name in ('c_bf16', 'd_f16'):
            line['a_spread_us'] = [a_lo, a_hi]
            line['median_within_or_below_a_spread'] = bool(np.median(v) <= a_hi)
        if name == 'c_bf16':
            line['gain_over_b_us'] = float(np.median(us['b_f32_plus_cast_bf16']) - np.median(v))
        lines.append(line)
        print(json.dumps(line), flush=True)
    lines.append({'row': 'state16_note', 'note': 'device time per call: HIP events around reps_per_round calls queued '
                  'behind two 8192^3 float32 matmuls, after 20 warm-up calls per variant; the variants alternate round '
                  'by round in one process; b = float32 render + copy_ into a preallocated bfloat16 batch; state_cache: whether '
                  'the bf16 / fp16 renders pass the state cache (--state-cache) or only the float32 render does (default)'})
    with open(args.out, 'w') as f:
        f.write(''.join(json.dumps(x) + '\n' for x in lines))


def bench_store(args):
    """A bf16 store of `capacity` stacks filled from the render of `envs` envs of `config` (256 agents),
    CHW: (a) render(out=ring) of all agents + store.index_copy_(0, dest, ring), today's route;
    (b) render_into(store, dest) of the same agents; (c) a host-chosen subset of a quarter of the agents
    rendered with slots= + the index_copy_; (d) render_into over all agents with the other three
    quarters' destinations at -1.  The method is bench_state16's: device time by HIP events around
    `reps` calls queued behind a blocking kernel, the variants alternating round by round in this
    process, each reporting its rounds' median, min and max.  No ratio is fixed in advance: (b) is
    compared with (a)'s min..max and (d) with (c)'s."""
    scenes = [synthetic.make_scene(args.config, e) for e in range(args.envs)]
    # --state-cache: render_into and the bf16 renders pass the batch's state cache (off by default: DESIGN.md section 5)
    b = batch.StateBatch(scenes, layout='chw', state_cache='all' if args.state_cache else True)
    dt = torch.bfloat16
    store = b.alloc_store(args.capacity, dtype=dt).zero_()
    check = torch.zeros_like(store)
    ring = b.alloc_state(dtype=dt)
    rs = np.random.RandomState(7)
    rows = rs.permutation(args.capacity)[:b.N].astype(np.int64)
    dest = torch.from_numpy(rows).to(b.device)
    sub = [int(k) for k in np.sort(rs.permutation(b.N)[:b.N // 4])]
    ring_sub = b.alloc_state(len(sub), dtype=dt)
    dest_sub = dest[torch.as_tensor(sub, device=b.device)].contiguous()
    masked = np.full(b.N, -1, dtype=np.int64)
    masked[sub] = rows[sub]
    dest_masked = torch.from_numpy(masked).to(b.device)

    def all_copy(st=store):
        b.render(out=ring)
        st.index_copy_(0, dest, ring)

    def sub_copy(st=store):
        b.render(out=ring_sub, slots=sub)
        st.index_copy_(0, dest_sub, ring_sub)
    variants = {'a_render_plus_index_copy': all_copy, 'b_render_into': lambda: b.render_into(store, dest),
                'c_subset_render_plus_index_copy': sub_copy,
                'd_render_into_masked': lambda: b.render_into(store, dest_masked)}
    # the routes agree before they are timed
    all_copy(check)
    b.render_into(store, dest)
    torch.cuda.synchronize()
    assert torch.equal(store.view(torch.int16), check.view(torch.int16))
    store.zero_()
    check.zero_()
    sub_copy(check)
    b.render_into(store, dest_masked)
    torch.cuda.synchronize()
    assert torch.equal(store.view(torch.int16), check.view(torch.int16))
    del check
    for f in variants.values():
        for _ in range(20):
            f()
    torch.cuda.synchronize()
    big = torch.randn(8192, 8192, device='cuda')
    s = torch.cuda.current_stream()
    us = {k: [] for k in variants}
    for _ in range(args.rounds):
        for name, f in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.mm(big, big)
            torch.mm(big, big)
            e0.record(s)
            for _ in range(args.reps):
                f()
            e1.record(s)
            torch.cuda.synchronize()
            us[name].append(e0.elapsed_time(e1) / args.reps * 1e3)
    from simaps import _lib
    _lib.check_faults()
    lines = []
    against = {'b_render_into': 'a_render_plus_index_copy', 'd_render_into_masked': 'c_subset_render_plus_index_copy'}
    for name, v in us.items():
        n = b.N if name[0] in 'ab' else len(sub)
        line = {'row': 'store', 'variant': name, 'config': args.config, 'agents_launched': b.N if name[0] != 'c' else n,
                'stacks_stored': n, 'channels': b.C, 'layout': 'chw', 'store_dtype': 'bfloat16',
                'store_capacity': args.capacity, 'median_us': float(np.median(v)), 'min_us': min(v), 'max_us': max(v),
                'rounds_us': [round(x, 3) for x in v], 'reps_per_round': args.reps,
                'state_cache': 'all' if args.state_cache else 'float32 render only'}
        if name in against:
            o = us[against[name]]
            line['against'] = against[name]
            line['against_spread_us'] = [min(o), max(o)]
            line['median_below_against_spread'] = bool(np.median(v) < min(o))
            line['gain_us'] = float(np.median(o) - np.median(v))
        lines.append(line)
        print(json.dumps(line), flush=True)
    lines.append({'row': 'store_note', 'note': 'device time per call: HIP events around reps_per_round calls queued '
                  'behind two 8192^3 float32 matmuls, after 20 warm-up calls per variant; the variants alternate round '
                  'by round in one process; a / c = render into a preallocated bf16 batch + store.index_copy_(0, dest, '
                  'batch); b / d = one simaps_get_state_into launch; the destination rows are a fixed random choice '
                  'among the store\'s rows; state_cache: whether these launches pass the state cache (--state-cache; maps '
                  'unchanged, so every launch after the first is a hit) or go without (default)'})
    with open(args.out, 'w') as f:
        f.write(''.join(json.dumps(x) + '\n' for x in lines))


def bench_remap(args):
    """The periodic re-map of one moving robot (RobotController.step -> update_map every 200
    simulation steps, envs.py:1401-1403): a single-frame simaps_ingest, end to end (host prep +
    upload + launch + synchronize, frame already on the device) and the two kernels alone."""
    from simaps import vector_env
    scenes = [synthetic.make_scene(args.config, e) for e in range(args.envs)]
    obs = vector_env.VectorEnvObservations(scenes, layout='chw')
    db, raw = synthetic.camera_images(scenes[3], 2, 'forward', seed=1)
    dep, seg = torch.as_tensor(db[None]).cuda(), torch.as_tensor(raw[None]).cuda()

    def step():
        obs.update_map([(3, 2)], dep, seg)
        torch.cuda.synchronize()
    for _ in range(5):
        step()
    ts = []
    for _ in range(300):
        t0 = time.perf_counter()
        step()
        ts.append(time.perf_counter() - t0)
    prep = obs.batch.prepare_ingest(dep, seg, camera='forward', slots=[obs.slot[(3, 2)]])
    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(s)
    for _ in range(100):
        obs.batch.launch_ingest(prep)
    e1.record(s)
    torch.cuda.synchronize()
    print(json.dumps({'row': 'remap_one_robot', 'config': args.config, 'frames_per_launch': 1,
                      'ms_end_to_end': float(np.median(ts)) * 1e3, 'kernel_ms': e0.elapsed_time(e1) / 100,
                      'note': 'update_map([(env, robot)], frame) + synchronize, median of 300; kernels: HIP events '
                              'over 100 back-to-back launches'}), flush=True)


def bench_ingest(args):
    """Ingest row: the two kernels alone (HIP events on the launch stream around K launches of the
    device half, inputs resident) and end to end (host packing + upload + launch), with an HBM
    roofline: algorithmic bytes per frame = 8 B per camera pixel (depth f32 + seg i32 read once)
    + 5 B per map pixel (the overhead f32 / occupancy u8 maps it may rewrite)."""
    import oracle
    from simaps import camera
    scenes = [synthetic.make_scene(args.config, e) for e in range(args.envs)]
    b = batch.StateBatch(scenes)
    kind = 'forward'
    frames = [synthetic.camera_images(scenes[e], a, kind, seed=e * 8 + a) for e, a in b.agents]
    dep = torch.as_tensor(np.stack([f[0] for f in frames])).cuda()
    seg = torch.as_tensor(np.stack([f[1] for f in frames])).cuda()
    dt_e2e = timed(lambda: b.ingest(dep, seg, camera=kind), args.steps, 3)
    prep = b.prepare_ingest(dep, seg, camera=kind)
    for _ in range(3):
        b.launch_ingest(prep)
    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    steps = max(args.steps, 50)
    torch.cuda.synchronize()
    e0.record(s)
    for _ in range(steps):
        b.launch_ingest(prep)
    e1.record(s)
    torch.cuda.synchronize()
    kern_ms = e0.elapsed_time(e1) / steps
    spec = camera.CAMERAS[kind]
    npix = spec.height_px * spec.width_px
    alg = b.N * (8 * npix + 5 * b.H * b.W)
    n, el = 0, 0.0
    for k, (e, a) in enumerate(b.agents):
        sc = scenes[e]
        r = sc['robots'][a]
        ov, oc = sc['overhead'][a].copy(), sc['occupancy'][a].copy()
        t0 = time.perf_counter()
        oracle.ingest(ov, oc, frames[k][0], frames[k][1], spec.params(r['position'][0], r['position'][1], r['heading']),
                      spec, synthetic.SEG_IDS, sc['receptacle_position'] is not None)
        el += time.perf_counter() - t0
        n += 1
        if el > args.cpu_budget:
            break
    print(json.dumps({'row': 'ingest', 'config': args.config, 'camera': kind, 'frames_per_launch': b.N,
                      'points_per_frame': npix, 'gpu_frames_per_s': b.N / (kern_ms * 1e-3),
                      'gpu_ms_per_launch': kern_ms, 'gpu_frames_per_s_end_to_end': b.N / dt_e2e,
                      'gpu_ms_end_to_end': dt_e2e * 1e3,
                      'roofline': {'bound': 'hbm', 'achieved': alg / (kern_ms * 1e-3) / 1e9, 'peak': 8000.0,
                                   'unit': 'GB/s', 'frac': alg / (kern_ms * 1e-3) / 1e9 / 8000.0,
                                   'algorithmic_bytes_per_frame': alg // b.N,
                                   'kernels': 'ingest_points_kernel + ingest_resolve_kernel'},
                      'cpu_oracle_frames_per_s': n / el, 'cpu_cores': 1,
                      'cpu_sample': '%d frames: capture_image points + argsort scatter + obstacle scatter' % n}),
          flush=True)


def bench_mixed(envs=64, steps=50):
    """`envs` envs of each BASELINE configuration (configs[0..4]; pushing_4-large_empty and
    lifting_2_throwing_2-large_empty share one), interleaved env by env, rendered by ONE
    MixedStateBatch launch vs one StateBatch launch per configuration back to back on the same
    stream.  Device time by HIP events over `steps` launches (sequences) after warm-up."""
    cfgs = ['lifting_1-small_empty', 'lifting_4-small_divider', 'pushing_4-large_empty',
            'lifting_2_throwing_2-large_empty', 'rescue_4-small_empty']
    scenes = [synthetic.make_scene(c, 1000 * k + e) for e in range(envs) for k, c in enumerate(cfgs)]
    mb = batch.MixedStateBatch(scenes)
    out = mb.alloc_state()
    groups = {}
    for s in scenes:
        groups.setdefault(batch.config_key(s), []).append(s)
    sbs = [batch.StateBatch(g) for g in groups.values()]
    outs = [b.alloc_state() for b in sbs]
    s = torch.cuda.current_stream()
    res = {}
    for name, f in (('mixed', lambda: mb.render(out)), ('per_config', lambda: [b.render(o) for b, o in zip(sbs, outs)])):
        for _ in range(5):
            f()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(steps):
            f()
        e1.record(s)
        torch.cuda.synchronize()
        res[name] = e0.elapsed_time(e1) / steps
    got = mb.states(out)
    env_of = {id(sc): i for i, sc in enumerate(scenes)}
    slot = {ea: k for k, ea in enumerate(mb.agents)}
    ok = all(torch.equal(got[slot[(env_of[id(b.scenes[e])], a)]], o[n])
             for b, o in zip(sbs, outs) for n, (e, a) in enumerate(b.agents))
    print(json.dumps({'row': 'mixed', 'configs': cfgs, 'envs_per_config': envs, 'stacks': mb.N,
                      'configurations_in_launch': len(mb.plan['cfgs']),
                      'mixed_ms': res['mixed'], 'per_config_ms': res['per_config'],
                      'mixed_stacks_per_s': mb.N / (res['mixed'] * 1e-3),
                      'per_config_stacks_per_s': mb.N / (res['per_config'] * 1e-3),
                      'per_config_launches': len(sbs), 'mixed_equals_per_config': bool(ok),
                      'note': 'HIP events over %d launches (sequences); inputs resident' % steps}), flush=True)


def bench_gridgraph_large(n=500, density=0.25, seed=505):
    """GridGraph(grid).shortest_path_image / shortest_path on an n x n random grid (obstacle density
    `density`), B = 1, 64 and 256 queries per launch (256: one query per CU), against the oracle's C SPFA (the reference's
    algorithm, 1 core; the reference's Cython SPFA runs at about the same speed, profiles/r2_cpu_calibration.json)."""
    import oracle
    rs = np.random.RandomState(seed)
    grid = (rs.random_sample((n, n)) > density).astype(np.uint8)
    free = np.argwhere(grid != 0)
    pick = lambda k: free[rs.randint(len(free), size=k)].astype(np.int32)  # noqa: E731
    g1 = torch.from_numpy(grid).cuda()
    rows = {}
    for B in (1, 64, 256):
        grids = g1.unsqueeze(0).expand(B, n, n).contiguous()
        srcs = torch.from_numpy(pick(B)).cuda()
        tg = pick(B)
        img = timed(lambda: batch.sssp_grid(grids, srcs), 3, 1)
        pth = timed(lambda: batch.launch_grid_paths(grids, srcs, torch.from_numpy(tg).cuda(), max_points=1024), 2, 1)
        rows[B] = (img, pth)
    s0, t0 = pick(1)[0], pick(1)[0]
    c0 = time.perf_counter()
    oracle.spfa_image(grid, tuple(s0))
    cpu_img = time.perf_counter() - c0
    c0 = time.perf_counter()
    oracle.grid_shortest_path(grid, tuple(s0), tuple(t0))
    cpu_path = time.perf_counter() - c0
    print(json.dumps({'row': 'gridgraph_large', 'grid': '%dx%d' % (n, n), 'obstacle_density': density,
                      'gpu_image_ms': {str(B): v[0] * 1e3 for B, v in rows.items()},
                      'gpu_images_per_s_at_64': 64 / rows[64][0], 'gpu_images_per_s_at_256': 256 / rows[256][0],
                      'gpu_path_ms': {str(B): v[1] * 1e3 for B, v in rows.items()},
                      'gpu_paths_per_s_at_64': 64 / rows[64][1], 'gpu_paths_per_s_at_256': 256 / rows[256][1],
                      'cpu_oracle_image_ms': cpu_img * 1e3, 'cpu_oracle_path_ms': cpu_path * 1e3, 'cpu_cores': 1,
                      'note': 'image: gl_tile_kernel (62 x 62 tiles in LDS, a queue of dirty tiles, four groups '
                              'of four waves; gl_sssp_kernel whole-window sweeps beyond 4,096 tiles); path: that '
                              'fixpoint + gl_path_kernel (one wave replays the SPFA, early exit at the target chain); '
                              'the SPFA is serial, one L2 round trip per pop'}), flush=True)


if __name__ == '__main__':
    if '--mixed' in sys.argv:
        bench_mixed()
        sys.exit(0)
    if '--gridgraph-large' in sys.argv:
        bench_gridgraph_large()
        sys.exit(0)
    if '--state16' in sys.argv:
        ap = argparse.ArgumentParser()
        ap.add_argument('--state16', action='store_true')
        ap.add_argument('--state-cache', action='store_true', help='the store / 16-bit launches pass the state cache')
        ap.add_argument('--config', default='lifting_4-small_divider')
        ap.add_argument('--envs', type=int, default=64)
        ap.add_argument('--rounds', type=int, default=15)
        ap.add_argument('--reps', type=int, default=100)
        ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'state16_bench.jsonl'))
        bench_state16(ap.parse_args())
        sys.exit(0)
    if '--store' in sys.argv:
        ap = argparse.ArgumentParser()
        ap.add_argument('--store', action='store_true')
        ap.add_argument('--state-cache', action='store_true', help='the store / 16-bit launches pass the state cache')
        ap.add_argument('--config', default='lifting_4-small_divider')
        ap.add_argument('--envs', type=int, default=64)
        ap.add_argument('--capacity', type=int, default=4096)
        ap.add_argument('--rounds', type=int, default=15)
        ap.add_argument('--reps', type=int, default=100)
        ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'store_bench.jsonl'))
        bench_store(ap.parse_args())
        sys.exit(0)
    if '--action-as' in sys.argv:  # only the rows of include/simaps_action_as.h (--action runs them too)
        bench_action_as(argparse.Namespace(config='lifting_4-small_divider', envs=64, awaiting=(64, 256), rounds=15,
                                           reps=100))
        sys.exit(0)
    if '--action' in sys.argv:
        bench_action(argparse.Namespace(config='lifting_4-small_divider', envs=64, steps=50, awaiting=(64, 256)))
        bench_action_as(argparse.Namespace(config='lifting_4-small_divider', envs=64, awaiting=(64, 256), rounds=15,
                                           reps=100))
        sys.exit(0)
    if '--env-step' in sys.argv:
        bench_env_step(argparse.Namespace(config='lifting_4-small_divider', envs=64, steps=50, all=False))
        bench_env_step(argparse.Namespace(config='lifting_4-small_divider', envs=64, steps=50, all=True))
        sys.exit(0)
    if '--dropin-only' in sys.argv:
        bench_dropin_step(argparse.Namespace(config='lifting_4-small_divider', envs=64, steps=50))
        bench_remap(argparse.Namespace(config='lifting_4-small_divider', envs=64))
        sys.exit(0)
    if '--ingest-only' in sys.argv:
        sys.argv.remove('--ingest-only')
    else:
        main()
        bench_dropin_step(argparse.Namespace(config='lifting_4-small_divider', envs=64, steps=50))
    bench_ingest(argparse.Namespace(config='lifting_4-small_divider', envs=64, steps=10, cpu_budget=8.0))
