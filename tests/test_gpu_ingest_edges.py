"""GPU: simaps_ingest / simaps_ingest_seq on the camera shapes, z ties, z orderings and body ids of
tests/ingest_cases.py (what each case is for is asserted on the CPU in tests/test_ingest_cases.py),
straight through the C ABI on a StateBatch's maps, which start as the scenes' own.

Each case runs tagged (epoch 7 on a key map full of stale keys of epoch 3) and zeroing (epoch 0 on
an all-zero key map).  Overhead bitwise and occupancy equal to oracle.ingest on every touched slot,
every other slot untouched, boxes[n][chunk] exact, and the key map equal to the numpy key model's on
every touched pixel (tagged; the winner's camera pixel, not only its code) or all zero (zeroing)."""
import numpy as np
import pytest
import torch

import ingest_cases as IC

pytestmark = pytest.mark.gpu

EPOCH, STALE = 7, 3


def _bitwise(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def _setup(c, mode):
    """A fresh batch on the scenes, the launch's device arguments, and the key map's contents before."""
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a GPU (run with -m gpu on an MI355X)')
    from simaps import _lib, batch
    b = batch.StateBatch(IC.scenes())
    slots = [b.agents.index((e, IC.AGENT)) for e in c.envs]
    n = len(slots)
    cam = b.ingest_buffers(c.spec, n)
    agents_d, _ = b.subset_descriptor(slots)
    ids = np.zeros(len(IC.SEEDS), dtype=_lib.SEG_IDS_DTYPE)
    for f in ('min_obstacle', 'max_obstacle', 'receptacle', 'min_cube', 'max_cube'):
        ids[f] = [d[f] for d in c.seg_ids]
    ids['has_receptacle'] = c.has_receptacle
    dev = dict(cam=cam, n=n, agents=agents_d, ids=batch._to_dev(ids, b.device),
               params=torch.from_numpy(np.ascontiguousarray(c.cam_params)).to(b.device),
               depth=torch.from_numpy(c.depth).to(b.device), seg=torch.from_numpy(c.seg_raw).to(b.device))
    keys0 = np.zeros((b.N, b.H, b.W), dtype=np.uint64)
    if mode == 'tagged':  # stale keys of an earlier epoch everywhere: they lose, and stay where nothing lands
        rng = np.random.default_rng(5)
        keys0 = (np.uint64(STALE) << np.uint64(56)) | rng.integers(0, 1 << 56, size=keys0.shape, dtype=np.uint64)
        b._keys.copy_(torch.from_numpy(keys0.view(np.int64)))
    return b, slots, dev, keys0


def _call(b, dev, epoch, seq=None):
    from simaps import _lib
    head = [b.cfg, dev['cam'], dev['n'], _lib.ptr(dev['agents']), _lib.ptr(dev['ids']), _lib.ptr(dev['params']),
            _lib.ptr(dev['depth']), _lib.ptr(dev['seg'])]
    tail = [_lib.ptr(b.overhead), _lib.ptr(b.occupancy), _lib.ptr(b._keys), _lib.ptr(b._boxes), epoch,
            _lib.stream_handle(torch.cuda.current_stream())]
    if seq is None:
        _lib.check(_lib.lib.simaps_ingest(*(head + tail)))
    else:
        seq_d = torch.tensor(seq, dtype=torch.int32, device=b.device)
        _lib.check(_lib.lib.simaps_ingest_seq(*(head + [_lib.ptr(seq_d), max(seq) + 1] + tail)))
    torch.cuda.synchronize()


def _check(name, mode, b, slots, keys0, c, ov, oc, ref, seq):
    from simaps import _lib
    sc = IC.scenes()
    got_ov, got_oc = b.overhead.cpu().numpy(), b.occupancy.cpu().numpy()
    keys = b._keys.cpu().numpy().view(np.uint64)
    for s, (e, a) in enumerate(b.agents):
        if s in slots:
            want_ov, want_oc = ov[e], oc[e]
        else:
            want_ov, want_oc = sc[e]['overhead'][a], sc[e]['occupancy'][a]
        d_ov = int((got_ov[s].view(np.int32) != np.asarray(want_ov, dtype=np.float32).view(np.int32)).sum())
        d_oc = int((got_oc[s] != want_oc).sum())
        assert d_ov == 0 and d_oc == 0, '%s %s: slot %d (env %d robot %d, %s): %d overhead, %d occupancy pixels differ' % (
            name, mode, s, e, a, 'touched' if s in slots else 'not touched', d_ov, d_oc)
    n, nch = len(slots), c.spec.chunks
    boxes = b._boxes[:n * nch * 4].cpu().numpy().reshape(n, nch, 4)
    for k in range(n):
        bad = np.nonzero((boxes[k] != ref.boxes[k]).any(axis=1))[0]
        assert len(bad) == 0, '%s %s: frame %d: %d of %d chunk boxes differ, first chunk %d: got %s, want %s' % (
            name, mode, k, len(bad), nch, bad[0], boxes[k][bad[0]].tolist(), ref.boxes[k][bad[0]].tolist())
    if mode == 'zero':
        assert not keys.any(), '%s: %d keys left after the zeroing launch' % (name, int((keys != 0).sum()))
    else:
        mk, hit = IC.model_keys(c, ref, EPOCH, seq)
        want = keys0.copy()
        for e in set(c.envs):
            s = b.agents.index((e, IC.AGENT))
            want[s][hit[e]] = mk[e][hit[e]]
        bad = np.argwhere(keys != want)
        if len(bad):
            s, i, j = bad[0]
            g, w = int(keys[s, i, j]), int(want[s, i, j])
            dec = lambda v: 'tag %d zkey %08x pixel %d code %d' % (v >> 56, (v >> 24) & 0xffffffff, ((v >> 4) & 0xfffff) - 1, v & 15)  # noqa: E731
            pytest.fail('%s: %d keys differ from the model (%d on touched pixels); first at slot %d (%d, %d): got %s, want %s'
                        % (name, len(bad), int(sum(hit[b.agents[q][0]][p, r] for q, p, r in bad if q in slots)), s, i, j, dec(g), dec(w)))
    _lib.check_faults()


@pytest.mark.parametrize('mode', ['tagged', 'zero'])
@pytest.mark.parametrize('name', IC.CASE_IDS)
def test_case_vs_oracle(name, mode):
    c, ov, oc, ref, _ = IC.solved(name)
    b, slots, dev, keys0 = _setup(c, mode)
    _call(b, dev, EPOCH if mode == 'tagged' else 0, c.seq)
    _check(name, mode, b, slots, keys0, c, ov, oc, ref, c.seq)


@pytest.mark.parametrize('mode', ['tagged', 'zero'])
@pytest.mark.parametrize('name', [k for k in IC.CASE_IDS if k.startswith('order')])
def test_order_reversed(name, mode):
    """The same frames with the first slot's order reversed equal the oracle applied in reversed order
    (which differs from the forward result: tests/test_ingest_cases.py)."""
    c, ov, oc, ref, seq = IC.solved(name, reverse=True)
    b, slots, dev, keys0 = _setup(c, mode)
    _call(b, dev, EPOCH if mode == 'tagged' else 0, seq)
    _check(name, mode, b, slots, keys0, c, ov, oc, ref, seq)


def test_prepare_ingest_takes_a_camera_spec():
    """StateBatch.prepare_ingest / launch_ingest with a CameraSpec of another size than the reference's
    in place of a camera name (the tie frames of 8 x 313 pixels; their poses are not CameraSpec.params',
    so the packed poses are replaced before the launch)."""
    from simaps import _lib, camera
    name = 'ties-8x313'
    c, ov, oc, ref, _ = IC.solved(name)
    b, slots, dev, keys0 = _setup(c, 'zero')
    spec = camera.CameraSpec('overhead', c.spec.aspect, c.spec.near, c.spec.far, height_px=8, width_px=313)
    with pytest.raises(ValueError, match=r'must be \(2, 8, 313\)'):
        b.prepare_ingest(c.depth[:, :, :-1], c.seg_raw[:, :, :-1], camera=spec, slots=slots)
    prep = b.prepare_ingest(c.depth, c.seg_raw, camera=spec, slots=slots)
    assert (prep['cam'].height_px, prep['cam'].width_px, prep['cam'].cx2) == (8, 313, c.spec.cx2)
    prep['params'] = dev['params']
    prep['ids'] = dev['ids']
    b.launch_ingest(prep)
    torch.cuda.synchronize()
    assert b._epoch == 1
    for k, s in enumerate(slots):
        assert _bitwise(b.overhead[s].cpu().numpy(), ov[c.envs[k]]) and np.array_equal(b.occupancy[s].cpu().numpy(), oc[c.envs[k]])
    _lib.check_faults()
