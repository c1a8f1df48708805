"""CPU: the ingest edge cases of tests/ingest_cases.py hold the conditions they exist for, asserted
from the reference alone with the counts in the messages, and on every case the numpy key model (max
of (monotone z, camera pixel) per map pixel) equals oracle.ingest -- so the GPU tests
(tests/test_gpu_ingest_edges.py) may compare the kernels' key map with the model's.  Also the ABI's
camera refusals at the ends of the accepted range, for both entry points.

No kernel is launched here."""
import ctypes
import os
import re

import numpy as np
import pytest

import ingest_cases as IC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'spatial-intention-maps_amd', 'csrc')


@pytest.mark.parametrize('name', IC.CASE_IDS)
def test_key_model_equals_oracle(name):
    """numpy key model == oracle.ingest: overhead bitwise, occupancy equal; the launch changes the maps."""
    c, ov, oc, ref, _ = IC.solved(name)
    mov, moc = IC.start_maps()
    IC.model_maps(mov, moc, c, ref)
    d_ov = int((mov.view(np.int32) != ov.view(np.int32)).sum())
    d_oc = int((moc != oc).sum())
    sov, soc = IC.start_maps()
    changed = int((sov.view(np.int32) != ov.view(np.int32)).sum()), int((soc != oc).sum())
    touched = int((ref.win_frame >= 0).sum())
    print('%s: %d map pixels touched, %d overhead / %d occupancy pixels changed; model vs oracle: %d / %d differ'
          % (name, touched, changed[0], changed[1], d_ov, d_oc))
    assert d_ov == 0 and d_oc == 0, '%s: model vs oracle.ingest: %d overhead, %d occupancy pixels differ' % (name, d_ov, d_oc)
    assert changed[0] > 0, '%s: the launch leaves the overhead maps as they were' % name
    assert c.spec.chunks == len(ref.boxes[0]) and c.depth.shape[1:] == (c.spec.height_px, c.spec.width_px)
    if name.startswith('order'):
        _, rov, _, _, rseq = IC.solved(name, reverse=True)
        d = int((rov.view(np.int32) != ov.view(np.int32)).sum())
        assert d > 0 and rseq[:3] == [2, 1, 0], '%s: forward and reversed order give the same overhead (%d differ)' % (name, d)
        e = c.envs[0]
        last_hit = np.zeros(ov.shape[1:], dtype=bool)
        last_hit[ref.frames[2].pi, ref.frames[2].pj] = True
        zmax = [np.full(ov.shape[1:], -np.inf) for _ in range(3)]
        for n in range(3):
            pts = IC.points(c.spec, c.cam_params[n], c.depth[n])
            np.maximum.at(zmax[n], (ref.frames[n].pi, ref.frames[n].pj), pts[:, 2])
        lower = sum(int(((zmax[n] <= zmax[2]) & last_hit & np.isfinite(zmax[n])).sum()) for n in (0, 1))
        both = sum(int((last_hit & np.isfinite(zmax[n])).sum()) for n in (0, 1))
        assert both >= 100 and lower == 0, '%s: %d pixels shared with the last frame, on %d the earlier frame is not higher' % (
            name, both, lower)
        assert (ref.win_frame[e][last_hit] == 2).all()


@pytest.mark.parametrize('name', ['widths-8x313', 'order-8x313', 'zorder-40x67'])
def test_model_keys_fields(name):
    """The expected key map packs tag << 56 | zkey << 24 | (k + 1) << 4 | code of each touched pixel's
    winner, 0 elsewhere; in an ordered launch the tag is the base plus the winning frame's seq."""
    c, ov, oc, ref, _ = IC.solved(name)
    keys, hit = IC.model_keys(c, ref, 7)
    assert keys.dtype == np.uint64 and hit.sum() > 0 and not keys[~hit].any()
    k = ((keys >> np.uint64(4)) & np.uint64(0xfffff)).astype(np.int64) - 1
    assert np.array_equal(k[hit], ref.win_k[hit]) and np.array_equal((keys & np.uint64(15)).astype(np.int64)[hit], ref.win_code[hit])
    tags = (keys >> np.uint64(56)).astype(np.int64)
    seq = np.asarray(c.seq if c.seq is not None else [0] * len(c.envs))
    assert np.array_equal(tags[hit], 7 + seq[ref.win_frame[hit]])
    zk = ((keys >> np.uint64(24)) & np.uint64(0xffffffff))
    for e in set(c.envs):
        for n in np.unique(ref.win_frame[e][hit[e]]):
            m = ref.win_frame[e] == n
            assert np.array_equal(zk[e][m], ref.frames[n].zk[ref.win_k[e][m]].astype(np.uint64))
    # the z keys order as the floats do, NaN last
    with IC.quiet(True):
        z = np.float32([-np.inf, -3e38, -1.5, -1e-45, 0.0, 1e-45, 2.5, 3e38, np.inf, np.nan])
    assert (np.diff(IC.zkeys(z).astype(np.int64)) > 0).all() and IC.zkeys(np.float32([-np.nan]))[0] == 0xffffffff


@pytest.mark.parametrize('name', sorted(IC.TIE_FRAMES))
def test_ties_condition(name):
    """Every point of a tie frame has one z, and at least 200 map pixels receive >= 2 points (of
    maximal z, as all are) with different codes: only the tie rule decides them."""
    c, ov, oc, ref, _ = IC.solved(name)
    H, W = ov.shape[1:]
    for n in IC.TIE_FRAMES[name]:
        f = ref.frames[n]
        assert len(np.unique(f.zk)) == 1, '%s frame %d: %d distinct z' % (name, n, len(np.unique(f.zk)))
        cell = f.pi * W + f.pj
        cnt = np.bincount(cell, minlength=H * W)
        cmin = np.full(H * W, 99)
        cmax = np.full(H * W, -1)
        np.minimum.at(cmin, cell, f.code)
        np.maximum.at(cmax, cell, f.code)
        decided = int(((cnt >= 2) & (cmin != cmax)).sum())
        print('%s frame %d: %d map pixels with >= 2 tied points of different codes' % (name, n, decided))
        assert decided >= 200, '%s frame %d: only %d map pixels with >= 2 tied points of different codes' % (name, n, decided)


def _areas(boxes):
    return (boxes[:, 1] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 2])


@pytest.mark.parametrize('name', ['modes-40x67', 'modes-8x640'])
def test_modes_condition(name):
    """Window mode (a chunk box of at most 2048 map pixels) and hash mode (more) both occur, and a
    hash-mode chunk has two touched cells on one slot (the collision path)."""
    c, ov, oc, ref, _ = IC.solved(name)
    assert (c.spec.width_px + 8 <= 320) == (name == 'modes-40x67')     # one camera per instantiation
    a0, a1 = _areas(ref.boxes[0]), _areas(ref.boxes[1])
    print('%s: chunk box areas: frame 0 %s, frame 1 %s' % (name, a0.tolist(), a1.tolist()))
    assert (a0 <= IC.WIN).all(), '%s: frame 0 chunk box areas %s, not all <= %d' % (name, a0.tolist(), IC.WIN)
    assert (a1 > IC.WIN).any(), '%s: frame 1 chunk box areas %s, none > %d' % (name, a1.tolist(), IC.WIN)
    f, colliding = ref.frames[1], 0
    for ch, (i0, i1, j0, j1) in enumerate(ref.boxes[1]):
        if (i1 - i0) * (j1 - j0) <= IC.WIN:
            continue
        s = slice(ch * IC.PTS, (ch + 1) * IC.PTS)
        cells = np.unique((f.pi[s] - i0) * (j1 - j0) + (f.pj[s] - j0))
        slots = cells % IC.HS
        colliding += len(cells) - len(np.unique(slots))
    print('%s: %d touched cells share a hash slot with another cell of their chunk' % (name, colliding))
    assert colliding >= 1, '%s: no two touched cells of a hash-mode chunk share a slot' % name


def test_window_constants_of_the_product_build():
    """SIMAPS_INGEST_WIN is 2048 unless a build overrides it, the product build does not, and the hash
    table has two thirds as many slots."""
    src = open(os.path.join(CSRC, 'simaps.hip')).read()
    assert re.search(r'#ifndef SIMAPS_INGEST_WIN\n#define SIMAPS_INGEST_WIN (\d+)\n#endif', src).group(1) == str(IC.WIN)
    assert 'constexpr int INGEST_WIN = SIMAPS_INGEST_WIN;' in src
    mk = open(os.path.join(CSRC, 'Makefile')).read()
    flags = re.search(r'^FLAGS\s*:=((?:.*\\\n)*.*)$', mk, re.M).group(1)
    assert 'SIMAPS_INGEST_WIN' not in flags, flags
    body = open(os.path.join(CSRC, 'ingest_points_body.inc')).read()
    assert 'constexpr int HS = INGEST_WIN * 2 / 3;' in body and IC.HS == IC.WIN * 2 // 3 == 1365


@pytest.mark.parametrize('name', ['ids-40x67', 'ids-8x313'])
def test_ids_condition(name):
    """Waves (512 consecutive camera pixels) without any id outside -1 .. 254 and waves with exactly one;
    every code the three envs' ranges can give the id set wins some map pixel, the top sums included."""
    c, ov, oc, ref, _ = IC.solved(name)
    npix = c.spec.npix
    clean = one = 0
    for n in range(len(c.envs)):
        seg = c.seg_raw[n].reshape(-1).astype(np.int64)
        out = (seg < -1) | (seg > 254)
        spans = [int(out[k:k + 512].sum()) for k in range(0, npix, 512)]
        clean, one = clean + spans.count(0), one + spans.count(1)
        assert set(spans) <= {0, 1}, spans
        assert not out[:IC.ids_split(npix)].any()
    # every code the ranges can produce from the id set, and which pairs (env, id) the frames hold
    can = set(int(IC.codes([r], IC.IDS_RANGES[e], IC.IDS_HAS[e])[0]) for e in range(3) for r in IC.ID_SET)
    won = set(int(v) for v in np.unique(ref.win_code[ref.win_frame >= 0]))
    in_maps = set(int(round(v * 8)) for v in np.unique(ov[ref.win_frame >= 0]))
    print('%s: %d wave spans without an out-of-range id, %d with exactly one; codes possible %s, winning %s'
          % (name, clean, one, sorted(can), sorted(won)))
    assert clean >= 1 and one >= 1, '%s: %d wave spans without, %d with exactly one out-of-range id' % (name, clean, one)
    assert won == can == in_maps, '%s: codes possible %s, winning %s, in the oracle maps %s' % (name, sorted(can), sorted(won), sorted(in_maps))
    assert {2, 9, 10} <= won, sorted(won)
    assert int((oc != IC.start_maps()[1]).sum()) > 0                      # the occupancy scatter shows
    # env 1 has no receptacle although its receptacle id is all over its frame
    assert (c.seg_raw[1] == IC.IDS_RANGES[1]['receptacle']).sum() > 100 and not c.has_receptacle[1]


@pytest.mark.parametrize('name', ['zorder-40x67', 'zorder-8x313'])
def test_zorder_condition(name):
    """NaN, inf and negative z each decide some map pixel, and points reach every map edge, pixel
    (0, 0) and row / column values past 2^31."""
    c, ov, oc, ref, _ = IC.solved(name)
    E, H, W = ov.shape
    nan_w = nan_neg = inf_w = neg_w = mixed = wrap_i = wrap_j = 0
    edges = np.zeros(4, dtype=np.int64)
    origin = 0
    for n in range(len(c.envs)):
        f, e = ref.frames[n], c.envs[n]
        with IC.quiet(True):
            pts = IC.points(c.spec, c.cam_params[n], c.depth[n])
            z = pts[:, 2]
            # finite row / column values at or past 2^31: numpy's cast wraps them to INT32_MIN (pixel 0),
            # where a saturating convert alone would clip them to the far edge
            vi, vj = np.floor(H / 2 - pts[:, 1] * IC.PPM), np.floor(W / 2 + pts[:, 0] * IC.PPM)
            wrap_i += int((np.isfinite(vi) & (vi >= 2.0 ** 31)).sum())
            wrap_j += int((np.isfinite(vj) & (vj >= 2.0 ** 31)).sum())
            assert (f.pi[np.isfinite(vi) & (vi >= 2.0 ** 31)] == 0).all() and (f.pj[np.isfinite(vj) & (vj >= 2.0 ** 31)] == 0).all()
        mine = ref.win_frame[e] == n
        zw = z[ref.win_k[e][mine]]
        nan_w += int(np.isnan(zw).sum())
        nan_neg += int((np.isnan(zw) & np.signbit(zw)).sum())
        inf_w += int(np.isinf(zw).sum())
        # a negative-z winner over a more negative point of the same pixel; pixels with both signs
        zmin = np.full(H * W, np.inf)
        zmax = np.full(H * W, -np.inf)
        fin = np.isfinite(z)
        np.minimum.at(zmin, (f.pi * W + f.pj)[fin], z[fin])
        np.maximum.at(zmax, (f.pi * W + f.pj)[fin], z[fin])
        zwin = np.full(H * W, np.nan)
        zwin[mine.reshape(-1)] = zw
        neg_w += int(((zwin < 0) & (zmin < zwin)).sum())
        mixed += int(((zwin > 0) & (zmin < 0)).sum())
        edges += [int((f.pi == 0).sum()), int((f.pi == H - 1).sum()), int((f.pj == 0).sum()), int((f.pj == W - 1).sum())]
        origin += int(((f.pi == 0) & (f.pj == 0)).sum())
        assert np.isnan(z).any() == (n == 0) and (np.isposinf(z).any() if n == 1 else np.isneginf(z).any())
    msg = ('%s: winners with NaN z %d (%d with the sign bit), inf z %d, negative z over a more negative point %d, positive '
           'over negative %d; points on edges i=0 %d, i=H-1 %d, j=0 %d, j=W-1 %d, on pixel (0, 0) %d; finite rows / columns '
           'past 2^31: %d / %d' % ((name, nan_w, nan_neg, inf_w, neg_w, mixed) + tuple(edges.tolist()) + (origin, wrap_i, wrap_j)))
    print(msg)
    assert nan_w >= 1 and nan_neg >= 1 and inf_w >= 1 and neg_w >= 1 and mixed >= 1, msg
    assert wrap_i >= 1 and wrap_j >= 1, msg
    assert (edges > 0).all() and origin > 0, (edges.tolist(), origin)


def test_row_and_column_table_reach():
    """Per shape: the largest row-table index a chunk reads (last pixel's row minus the chunk's first
    row; 31 is the table's last entry) and how many 8-pixel lane segments wrap to the next camera row
    (they read the column table's wrapped copies and switch rows).  40 x 67 stays one short of the
    table's end, 1162 x 67 reaches it; every shape but the widths that 8 divides has wrapping lanes."""
    reach, wraps = {}, {}
    for name in IC.CASE_IDS:
        s = IC.case(name).spec
        k0 = np.arange(0, s.npix, IC.PTS)
        last = np.minimum(k0 + IC.PTS, s.npix) - 1
        reach[name] = int((last // s.width_px - k0 // s.width_px).max())
        l0 = np.arange(0, s.npix - 7, 8)                                   # full lanes
        wraps[name] = int(((l0 % s.width_px) > s.width_px - 8).sum())
    print('largest row-table index per shape: %s' % reach)
    print('lane segments that wrap rows per shape: %s' % wraps)
    assert reach['widths-40x67'] == 30 and reach['rows-1162x67'] == 31 and max(reach.values()) == 31
    assert reach['widths-3x1024'] == 1 and reach['boxes64-130x1024'] == 1
    for name, w in wraps.items():
        assert (w > 0) == (IC.case(name).spec.width_px % 8 != 0), (name, w)


def test_unaligned_and_chunk_counts():
    """The shapes' pixel counts take every residue mod 4, and the chunk counts are the ones named."""
    from simaps import _lib
    res = {}
    for name in IC.CASE_IDS:
        s = IC.case(name).spec
        assert _lib.lib.simaps_ingest_chunks(s.height_px, s.width_px) == s.chunks, name
        if name.startswith('unaligned'):
            res.setdefault(s.npix % 4, []).append((s.npix, s.chunks, s.npix % IC.PTS))
            assert len(IC.case(name).envs) == 3
    print('unaligned shapes by NP %% 4: %s' % res)
    assert sorted(res) == [0, 1, 2, 3]
    assert all(t == 0 for _, _, t in res[0]) and any(ch == 1 for r in (1, 2, 3) for _, ch, _ in res[r])
    assert [IC.case('boxes64-%s' % s).spec.chunks for s in ('128x1024', '130x1024')] == [64, 65]
    assert IC.case('boxes64+ties-1023x1024').spec.chunks == 512


# ---- the ABI's camera range, both entry points ---------------------------------------------------
D = ctypes.c_void_p(0x1000)   # never dereferenced: every call below fails its checks first


def _ingest(L, seq, Hc, Wc):
    from simaps import batch, constants as K
    s = IC.Spec(Hc, Wc)
    cfg = batch.make_config(dict(K.DEFAULT_FLAGS), 1.0, 0.5)
    cam = L.Camera(s.height_px, s.width_px, s.near, s.far, s.cx2, s.cy2)
    head, tail = [cfg, cam, 1, D, D, D, D, D], [D, D, D, D, 1, None]
    if seq:
        return L.lib.simaps_ingest_seq(*(head + [D, 2] + tail))
    return L.lib.simaps_ingest(*(head + tail))


@pytest.mark.parametrize('seq', [False, True], ids=['ingest', 'ingest_seq'])
def test_camera_range_refusals(seq):
    from simaps import _lib as L
    err = L.lib.simaps_last_error
    for Wc in (66, 1025):
        assert _ingest(L, seq, 8, Wc) == L.EUNSUPPORTED, Wc
        assert b'camera width %d outside [67, 1024]' % Wc in err()
    assert _ingest(L, seq, 1024, 1024) == L.EUNSUPPORTED
    assert b'camera frame of 1048576 pixels' in err()
    assert _ingest(L, seq, 15651, 67) == L.EUNSUPPORTED and b'1048617 pixels' in err()   # the first count past 2^20 at width 67
    assert L.lib.simaps_ingest_chunks(1023, 1024) == 512
    assert L.lib.simaps_ingest_chunks(1024, 1024) == 512                  # (the count alone is no acceptance)
    assert L.lib.simaps_ingest_chunks(40, 67) == 2


def test_camera_spec_takes_a_size():
    """CameraSpec keeps the reference sizes by default and takes another one; prepare_ingest accepts
    the object in place of a name (checked on the GPU)."""
    from simaps import camera
    assert (camera.FORWARD.height_px, camera.FORWARD.width_px) == (156, 277)
    assert (camera.OVERHEAD.height_px, camera.OVERHEAD.width_px) == (156, 156)
    s = camera.CameraSpec('overhead', 313 / 8, 0.001, 10.0, height_px=8, width_px=313)
    t = IC.Spec(8, 313)
    assert (s.height_px, s.width_px, s.cx2, s.cy2) == (8, 313, t.cx2, t.cy2)
    assert s.params(0.1, 0.2, 0.3) == camera.OVERHEAD.params(0.1, 0.2, 0.3)
