"""GPU tests of the ordered multi-frame ingest (include/simaps_ingest_seq.h, StateBatch.prepare_ingest
ordered=True, VectorEnvObservations.queue_map_update / flush_map_updates) against the oracle's
per-frame ingest applied frame by frame.

Scenario (tests/test_gpu_dropin.py::test_periodic_remap_successive_frames): lifting_4-small_divider,
seeds 330+e, robot (2, 1) driving 2 cm and turning 10 degrees per re-map, frame seeds 900+k; the
reference's 156 x 277 forward camera; at most 8 frames per launch."""
import numpy as np
import pytest
import torch

import oracle as O

pytestmark = pytest.mark.gpu

E, A = 2, 1          # the moving robot
OTHER = (0, 3)       # a second robot with frames of its own (its pose stays the scene's)


def _bitwise(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.fixture(scope='module')
def P():
    """The scenario, computed once: scenes, the moving robot's 6 poses and frames (4 of the periodic
    re-map plus 2 more for the multi-launch tests), one frame of OTHER, and a helper that applies
    frames through the oracle."""
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a GPU (run with -m gpu on an MI355X)')
    from simaps import camera, synthetic

    class S:
        pass
    p = S()
    p.spec = camera.CAMERAS['forward']
    p.scenes = [synthetic.make_scene('lifting_4-small_divider', 330 + e) for e in range(4)]
    sc = p.scenes[E]
    x0, y0, h0 = sc['robots'][A]['position'][0], sc['robots'][A]['position'][1], sc['robots'][A]['heading']
    p.poses, p.depth, p.seg = [], [], []
    for k in range(6):
        pose = (x0 + 0.02 * k * np.cos(h0), y0 + 0.02 * k * np.sin(h0), h0 + np.radians(10) * k)
        moved = dict(sc, robots=[dict(rb) for rb in sc['robots']])
        moved['robots'][A]['position'] = (pose[0], pose[1], 0)
        moved['robots'][A]['heading'] = pose[2]
        db, raw = synthetic.camera_images(moved, A, 'forward', seed=900 + k)
        p.poses.append(pose), p.depth.append(db), p.seg.append(raw.astype(np.int32))
    ro = p.scenes[OTHER[0]]['robots'][OTHER[1]]
    p.other_pose = (ro['position'][0], ro['position'][1], ro['heading'])
    p.other_depth, p.other_seg = synthetic.camera_images(p.scenes[OTHER[0]], OTHER[1], 'forward', seed=950)
    p.other_seg = p.other_seg.astype(np.int32)

    def start(e=E, a=A):
        return p.scenes[e]['overhead'][a].copy(), p.scenes[e]['occupancy'][a].copy()

    def apply(ov, oc, frames, e=E):
        """frames: [(depth, seg, pose), ...] applied to (ov, oc) in order, in place."""
        for db, raw, pose in frames:
            O.ingest(ov, oc, db, raw, p.spec.params(*pose), p.spec, synthetic.SEG_IDS,
                     p.scenes[e]['receptacle_position'] is not None)
        return ov, oc

    p.start, p.apply = start, apply
    p.frame = lambda k: (p.depth[k], p.seg[k], p.poses[k])
    p.fwd = apply(*start(), [p.frame(k) for k in range(4)])
    p.rev = apply(*start(), [p.frame(k) for k in (3, 2, 1, 0)])
    return p


def _batch(P, context=None):
    from simaps import batch
    b = batch.StateBatch(P.scenes, context=context)
    return b, b.agents.index((E, A))


def _check_slot(b, slot, ref, what=''):
    ov, oc = ref
    assert _bitwise(b.overhead[slot].cpu().numpy(), ov), what
    assert np.array_equal(b.occupancy[slot].cpu().numpy(), oc), what


def _check_untouched(P, b, touched):
    ov, oc = b.overhead.cpu().numpy(), b.occupancy.cpu().numpy()
    for n, (e, a) in enumerate(b.agents):
        if n not in touched:
            assert _bitwise(ov[n], P.scenes[e]['overhead'][a]) and np.array_equal(oc[n], P.scenes[e]['occupancy'][a]), (e, a)


def _prep4(P, b, slot):
    return b.prepare_ingest(np.stack(P.depth[:4]), np.stack(P.seg[:4]), slots=[slot] * 4, poses=P.poses[:4], ordered=True)


def _seq_call(b, prep, epoch, seq='prep', num_seq=None, twin=None):
    """simaps_ingest_seq straight through the C ABI, on the batch's maps and key map."""
    from simaps import _lib
    seq = prep['seq'] if isinstance(seq, str) else seq
    args = [b.cfg, prep['cam'], prep['n'], _lib.ptr(prep['agents']), _lib.ptr(prep['ids']), _lib.ptr(prep['params']),
            _lib.ptr(prep['depth']), _lib.ptr(prep['seg']), _lib.ptr(seq), prep['num_seq'] if num_seq is None else num_seq,
            _lib.ptr(b.overhead), _lib.ptr(b.occupancy), _lib.ptr(b._keys), _lib.ptr(b._boxes), epoch,
            _lib.stream_handle(torch.cuda.current_stream())]
    _lib.check(_lib.lib.simaps_ingest_seq(*args))
    torch.cuda.synchronize()


def _tags(b):
    return set(int(x) for x in np.unique(b._keys.cpu().numpy().view(np.uint64) >> np.uint64(56)))


def test_order_within_one_launch(P):
    """Four frames of one slot in ONE ordered launch equal the oracle applying them in order; with seq
    reversed, the oracle in reverse order.  The two oracle results differ, so an order-blind kernel
    cannot pass both."""
    d_ov = int((P.fwd[0].view(np.int32) != P.rev[0].view(np.int32)).sum())
    d_oc = int((P.fwd[1] != P.rev[1]).sum())
    print('forward vs reverse oracle: %d overhead pixels, %d occupancy pixels differ' % (d_ov, d_oc))
    assert d_ov > 0
    b, slot = _batch(P)
    prep = _prep4(P, b, slot)
    assert prep['num_seq'] == 4 and prep['seq'].cpu().tolist() == [0, 1, 2, 3]
    ver = b._map_ver.copy()
    b.launch_ingest(prep)
    torch.cuda.synchronize()
    assert b._epoch == 4 and _tags(b) <= {0, 1, 2, 3, 4}
    assert (b._map_ver - ver).tolist() == [int(n == slot) for n in range(b.N)]   # once per touched slot
    _check_slot(b, slot, P.fwd)
    _check_untouched(P, b, {slot})
    b2, _ = _batch(P)
    prep2 = _prep4(P, b2, slot)
    prep2['seq'] = torch.tensor([3, 2, 1, 0], dtype=torch.int32, device=b2.device)
    b2.launch_ingest(prep2)
    torch.cuda.synchronize()
    _check_slot(b2, slot, P.rev)
    _check_untouched(P, b2, {slot})


def test_unordered_prepare_still_refuses_repeated_slots(P):
    b, slot = _batch(P)
    with pytest.raises(ValueError, match='one frame per map slot and launch'):
        b.prepare_ingest(np.stack(P.depth[:2]), np.stack(P.seg[:2]), slots=[slot, slot])


def test_interleaved_slots(P):
    """Three slots with 3, 1 and 0 frames in one launch; the frames of the first are not adjacent and
    seq is not monotone in n.  Each slot equals its own in-order oracle."""
    b, slot = _batch(P)
    other = b.agents.index(OTHER)
    # array order: A's third, OTHER's only, A's first, A's second frame
    dep = np.stack([P.depth[2], P.other_depth, P.depth[0], P.depth[1]])
    seg = np.stack([P.seg[2], P.other_seg, P.seg[0], P.seg[1]])
    poses = [P.poses[2], P.other_pose, P.poses[0], P.poses[1]]
    prep = b.prepare_ingest(dep, seg, slots=[slot, other, slot, slot], poses=poses, ordered=True)
    assert prep['num_seq'] == 3
    seq = torch.tensor([2, 0, 0, 1], dtype=torch.int32, device=b.device)
    _seq_call(b, prep, 1, seq=seq)
    _check_slot(b, slot, P.apply(*P.start(), [P.frame(0), P.frame(1), P.frame(2)]))
    _check_slot(b, other, P.apply(*P.start(*OTHER), [(P.other_depth, P.other_seg, P.other_pose)], e=OTHER[0]))
    _check_untouched(P, b, {slot, other})       # the slot with no frame among them


def test_single_frame_is_simaps_ingest(P):
    """num_seq == 1 with a NULL seq equals simaps_ingest on the same inputs: both maps and the key
    map bit for bit."""
    from simaps import synthetic
    got = []
    for ordered in (True, False):
        b, _ = _batch(P)
        f = [synthetic.camera_images(P.scenes[e], a, 'forward', seed=40 + n) for n, (e, a) in enumerate(b.agents[:6])]
        prep = b.prepare_ingest(np.stack([x[0] for x in f]), np.stack([x[1] for x in f]).astype(np.int32),
                                slots=list(range(6)))
        if ordered:
            _seq_call(b, dict(prep, seq=None, num_seq=1), 3)
        else:
            b._epoch = 2
            b.launch_ingest(prep)               # simaps_ingest at epoch 3
            torch.cuda.synchronize()
        got.append((b.overhead.cpu().numpy(), b.occupancy.cpu().numpy(), b._keys.cpu().numpy()))
    assert _bitwise(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
    assert np.array_equal(got[0][2], got[1][2]) and got[0][2].any()


def test_tags_across_launches_on_one_key_map(P):
    """num_seq 3 at epoch 1, then num_seq 2 at epoch 4, then plain simaps_ingest at epoch 6, all on
    one key map: exact after each."""
    from simaps import _lib
    b, slot = _batch(P)
    ref = P.start()
    prep = b.prepare_ingest(np.stack(P.depth[:3]), np.stack(P.seg[:3]), slots=[slot] * 3, poses=P.poses[:3], ordered=True)
    _seq_call(b, prep, 1)
    _check_slot(b, slot, P.apply(*ref, [P.frame(k) for k in range(3)]), 'launch 1')
    assert _tags(b) <= {0, 1, 2, 3}
    prep = b.prepare_ingest(np.stack(P.depth[3:5]), np.stack(P.seg[3:5]), slots=[slot] * 2, poses=P.poses[3:5], ordered=True)
    _seq_call(b, prep, 4)
    _check_slot(b, slot, P.apply(*ref, [P.frame(3), P.frame(4)]), 'launch 2')
    assert _tags(b) <= {0, 1, 2, 3, 4, 5}
    prep = b.prepare_ingest(P.depth[5][None], P.seg[5][None], slots=[slot], poses=P.poses[5:6])
    _lib.check(_lib.lib.simaps_ingest(
        b.cfg, prep['cam'], 1, _lib.ptr(prep['agents']), _lib.ptr(prep['ids']), _lib.ptr(prep['params']),
        _lib.ptr(prep['depth']), _lib.ptr(prep['seg']), _lib.ptr(b.overhead), _lib.ptr(b.occupancy), _lib.ptr(b._keys),
        _lib.ptr(b._boxes), 6, _lib.stream_handle(torch.cuda.current_stream())))
    torch.cuda.synchronize()
    _check_slot(b, slot, P.apply(*ref, [P.frame(5)]), 'launch 3')
    _check_untouched(P, b, {slot})


def test_statebatch_epochs_and_wrap(P):
    """StateBatch's tag bookkeeping across mixed plain and ordered launches: an ordered launch takes
    num_seq epochs; when its last tag would pass 255 the key map is zeroed first and the count
    restarts.  Exact throughout."""
    b, slot = _batch(P)
    ref = P.start()
    b.ingest(P.depth[0][None], P.seg[0][None], slots=[slot])        # plain: epoch 1 (the descriptor's pose = pose 0)
    P.apply(*ref, [P.frame(0)])
    assert b._epoch == 1
    b._epoch = 250                                                  # as after 250 launches
    two = lambda i, j: b.prepare_ingest(np.stack([P.depth[i], P.depth[j]]), np.stack([P.seg[i], P.seg[j]]),  # noqa: E731
                                        slots=[slot, slot], poses=[P.poses[i], P.poses[j]], ordered=True)
    b.launch_ingest(two(1, 2))                                      # tags 251, 252
    assert b._epoch == 252
    b.launch_ingest(_prep4(P, b, slot))                             # 253 + 3 > 255: the wrap path, tags 1 .. 4
    assert b._epoch == 4
    torch.cuda.synchronize()
    assert _tags(b) <= {0, 1, 2, 3, 4}
    _check_slot(b, slot, P.apply(*ref, [P.frame(1), P.frame(2)] + [P.frame(k) for k in range(4)]), 'after the wrap')
    b.ingest(P.depth[5][None], P.seg[5][None], slots=[slot])        # plain again: epoch 5
    assert b._epoch == 5
    b._epoch = 254
    b.launch_ingest(two(4, 3))                                      # 255 + 1 > 255: wraps, tags 1, 2
    assert b._epoch == 2
    torch.cuda.synchronize()
    pose0 = P.poses[0]
    _check_slot(b, slot, P.apply(*ref, [(P.depth[5], P.seg[5], pose0), P.frame(4), P.frame(3)]), 'second wrap')
    _check_untouched(P, b, {slot})


def test_zero_mode_and_graph_replay(P):
    """After an epoch-0 ordered launch the key map is all zero.  An ordered launch with two frames
    per slot, captured into a graph, is replayed twice with new frame contents copied into the
    captured buffers: each replay equals the oracle."""
    b, slot = _batch(P)
    prep = _prep4(P, b, slot)
    _seq_call(b, prep, 0)
    assert not b._keys.any().item()
    _check_slot(b, slot, P.fwd)
    # capture: slot A frames (0, 1), OTHER twice (its own frame, then A's frame 2 seen from OTHER's pose)
    b, slot = _batch(P)
    other = b.agents.index(OTHER)
    dep = np.stack([P.depth[0], P.other_depth, P.depth[1], P.depth[2]])
    seg = np.stack([P.seg[0], P.other_seg, P.seg[1], P.seg[2]])
    poses = [P.poses[0], P.other_pose, P.poses[1], P.other_pose]
    prep = b.prepare_ingest(dep, seg, slots=[slot, other, slot, other], poses=poses, ordered=True)
    assert prep['num_seq'] == 2
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        b.launch_ingest(prep)
    assert b._epoch == 0 and b._zero_mode
    ref_a, ref_o = P.start(), P.start(*OTHER)
    for rep, ks in enumerate(((0, 1, 2), (3, 4, 5))):
        if rep:
            dep = np.stack([P.depth[ks[0]], P.other_depth, P.depth[ks[1]], P.depth[ks[2]]])
            seg = np.stack([P.seg[ks[0]], P.other_seg, P.seg[ks[1]], P.seg[ks[2]]])
            prep['depth'].copy_(torch.from_numpy(dep))
            prep['seg'].copy_(torch.from_numpy(seg))
        g.replay()
        torch.cuda.synchronize()
        # (the captured poses stay: frames ks[0], ks[1] from poses 0, 1; OTHER's two from its own pose)
        P.apply(*ref_a, [(P.depth[ks[0]], P.seg[ks[0]], P.poses[0]), (P.depth[ks[1]], P.seg[ks[1]], P.poses[1])])
        P.apply(*ref_o, [(P.other_depth, P.other_seg, P.other_pose), (P.depth[ks[2]], P.seg[ks[2]], P.other_pose)],
                e=OTHER[0])
        _check_slot(b, slot, ref_a, 'replay %d' % rep)
        _check_slot(b, other, ref_o, 'replay %d' % rep)
        assert not b._keys.any().item()
    _check_untouched(P, b, {slot, other})


def _obs(P, **kw):
    from simaps import batch, vector_env
    obs = vector_env.VectorEnvObservations(P.scenes, layout='hwc', **kw)
    return obs, batch.descriptor_arrays(P.scenes), obs.batch._robot_off[E] + A, obs.slot[(E, A)]


def test_dropin_queue_and_auto_flush(P):
    """The periodic re-map through queue_map_update x 4 with update_arrays between: nothing is
    launched until get_state flushes (pending 4 -> 0); the robot's maps and state are the oracle's."""
    from simaps import vector_env
    obs, arrays, r, slot = _obs(P)
    for k in range(4):
        arrays['pose'][r] = P.poses[k]
        obs.update_arrays(**arrays)
        obs.queue_map_update([(E, A)], P.depth[k][None], P.seg[k][None])
        assert obs.pending_map_updates == k + 1
    torch.cuda.synchronize()
    assert _bitwise(obs.batch.overhead[slot].cpu().numpy(), P.scenes[E]['overhead'][A])      # nothing launched yet
    st = obs.get_state(awaiting=[[False] * 4, [False] * 4, [k == A for k in range(4)], [False] * 4], numpy=True)
    assert obs.pending_map_updates == 0
    _check_slot(obs.batch, slot, P.fwd)
    _check_untouched(P, obs.batch, {slot})
    sc = P.scenes[E]
    moved = dict(sc, robots=[dict(rb) for rb in sc['robots']])
    moved['robots'][A]['position'] = (P.poses[3][0], P.poses[3][1], 0)
    moved['robots'][A]['heading'] = P.poses[3][2]
    moved['overhead'], moved['occupancy'] = sc['overhead'].copy(), sc['occupancy'].copy()
    moved['overhead'][A], moved['occupancy'][A] = P.fwd
    groups = vector_env.robot_groups(sc)
    g = [gi for gi, grp in enumerate(groups) if A in grp][0]
    assert _bitwise(st[E][g][groups[g].index(A)], O.agent_state(moved, A))


def test_dropin_queue_then_immediate_and_small_queue(P):
    """A queued frame followed by an immediate update_map of the same robot keeps the order; a queue
    of capacity 2 given three frames flushes by itself and stays exact."""
    obs, arrays, r, slot = _obs(P)
    # frames 3 then 0: the reverse-order pair, whose result differs from 0 then 3
    arrays['pose'][r] = P.poses[3]
    obs.update_arrays(**arrays)
    obs.queue_map_update([(E, A)], P.depth[3][None], P.seg[3][None])
    arrays['pose'][r] = P.poses[0]
    obs.update_arrays(**arrays)
    obs.update_map([(E, A)], P.depth[0][None], P.seg[0][None])
    assert obs.pending_map_updates == 0
    torch.cuda.synchronize()
    _check_slot(obs.batch, slot, P.apply(*P.start(), [P.frame(3), P.frame(0)]))
    obs, arrays, r, slot = _obs(P, map_queue=2)
    pending = []
    for k in (2, 1, 0):
        arrays['pose'][r] = P.poses[k]
        obs.update_arrays(**arrays)
        obs.queue_map_update([(E, A)], P.depth[k][None], P.seg[k][None])
        pending.append(obs.pending_map_updates)
    assert pending == [1, 2, 1]                                     # the third frame found the queue full
    obs.flush_map_updates()
    assert obs.pending_map_updates == 0
    torch.cuda.synchronize()
    _check_slot(obs.batch, slot, P.apply(*P.start(), [P.frame(2), P.frame(1), P.frame(0)]))
    _check_untouched(P, obs.batch, {slot})


def test_through_a_context(P):
    """The ordered launch through a Context (simaps_ctx_ingest_seq) gives the same bytes."""
    from simaps import context
    with context.Context() as ctx:
        b, slot = _batch(P, context=ctx)
        b.launch_ingest(_prep4(P, b, slot))
        torch.cuda.synchronize()
        _check_slot(b, slot, P.fwd)
        _check_untouched(P, b, {slot})
        ctx.check_faults()
        del b
