"""Shared case builders of the ingest edge tests (tests/test_ingest_cases.py on the CPU,
tests/test_gpu_ingest_edges.py on the GPU): camera shapes, z ties, z orderings and body ids that
simaps_ingest / simaps_ingest_seq accept (include/simaps.h, include/simaps_ingest_seq.h) and that
synthetic.camera_images never produces.

A case is one launch: one camera shape, n frames, each frame onto the map slot of robot 0 of env
`envs[n]` of three lifting_4-small_divider scenes (184 x 232 maps).  Every frame is built here.

Besides oracle.ingest (the arbiter of the maps) the module holds a numpy model of the kernels' key
rule: per map pixel the winner is the point with the largest (z made unsigned-monotone with NaN last,
camera pixel index), and its key is tag << 56 | zkey << 24 | (k + 1) << 4 | code.  The CPU tests
assert that this model and the oracle agree on every case, so the GPU tests may compare the key map
with the model's: that pins the winner's camera pixel, not only its code."""
import collections
import contextlib
import functools
import math
import warnings

import numpy as np

import oracle as O

CONFIG = 'lifting_4-small_divider'
SEEDS = (330, 331, 332)      # one scene per env; frames go to robot AGENT of an env
AGENT = 0
PTS = 2048                   # camera pixels per point-pass chunk (simaps_ingest_chunks)
WIN = 2048                   # SIMAPS_INGEST_WIN of the product build: LDS window entries
HS = WIN * 2 // 3            # slots of the hash mode's direct-mapped table
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
PPM = O.PPM

Case = collections.namedtuple('Case', 'spec cam_params depth seg_raw seg_ids has_receptacle name envs seq nonfinite')
FrameRef = collections.namedtuple('FrameRef', 'pi pj code zk boxes')
Ref = collections.namedtuple('Ref', 'frames boxes win_frame win_k win_code')


class Spec:
    """The camera constants simaps_camera and oracle.ingest read."""

    def __init__(self, height_px, width_px, aspect=None, near=0.001, far=10.0):
        self.height_px, self.width_px = int(height_px), int(width_px)
        self.aspect = width_px / height_px if aspect is None else aspect
        self.near, self.far = near, far
        limit_y = math.tan(math.radians(60 / 2))
        limit_x = limit_y * self.aspect
        self.cx2, self.cy2 = 2 * limit_x, 2 * limit_y

    @property
    def npix(self):
        return self.height_px * self.width_px

    @property
    def chunks(self):
        return -(-self.npix // PTS)


@functools.lru_cache(maxsize=None)
def scenes():
    from simaps import synthetic
    return [synthetic.make_scene(CONFIG, s) for s in SEEDS]


def default_ids():
    from simaps import synthetic
    return [dict(synthetic.SEG_IDS) for _ in SEEDS], [1] * len(SEEDS)


def start_maps():
    """(overhead [E, H, W] f32, occupancy [E, H, W] u8): the scenes' own maps of robot AGENT."""
    sc = scenes()
    return (np.stack([s['overhead'][AGENT] for s in sc]).astype(np.float32),
            np.stack([s['occupancy'][AGENT] for s in sc]).astype(np.uint8))


# ---- frame design (float64; nothing here has to be exact: the frames are inputs) ----------------
def _rays64(spec, params):
    p = np.asarray(params, dtype=np.float64)
    cp = p[0:3]
    pr = p[3:6] - cp
    pr = pr / np.linalg.norm(pr)
    up = p[6:9] - np.dot(p[6:9], pr) * pr
    up = up / np.linalg.norm(up)
    right = np.cross(pr, up)
    px = spec.cx2 * (np.arange(spec.width_px) / spec.width_px - 0.5)
    py = spec.cy2 * (0.5 - (np.arange(spec.height_px) + 1) / spec.height_px)
    return cp, pr + px[None, :, None] * right + py[:, None, None] * up


def depth_buffer(spec, dep):
    """The depth buffer value(s) whose depth along the principal axis is `dep`."""
    return np.asarray((spec.far - spec.far * spec.near / np.asarray(dep, dtype=np.float64)) / (spec.far - spec.near),
                      dtype=np.float32)


def plane_depth(spec, params, z):
    """Depth buffer [Hc, Wc] whose points lie (up to rounding) at height z [Hc, Wc]."""
    cp, t = _rays64(spec, params)
    return depth_buffer(spec, (z - cp[2]) / t[..., 2])


def look_down(x, y, height, heading, tilt=(0.0, 0.0)):
    """An overhead-type pose (OverheadCamera, envs.py:1974-1978) at `height`, its target moved by tilt."""
    return [x, y, height, x + tilt[0], y + tilt[1], 0.0, math.cos(heading), math.sin(heading), 0.0]


def height_for(spec, density):
    """Camera height at which `density` camera rows fall on one map row below the camera."""
    return spec.height_px / (density * PPM * spec.cy2)


GENERIC_IDS = (-1, 0, 1, 2, 3, 4, 99, 10, 11)


def generic_frame(spec, rng, density, heading, x=0.0, y=0.0, levels=(0.0, 0.1, 0.3), ids=GENERIC_IDS, tilt=True):
    """A tilted look-down camera over a floor of 4 x 4-pixel blocks at heights levels * camera height,
    random body ids."""
    h = height_for(spec, density)
    params = look_down(x, y, h, heading, (0.1 * h, -0.05 * h) if tilt else (0.0, 0.0))
    Hc, Wc = spec.height_px, spec.width_px
    lv = rng.choice(np.asarray(levels), size=(-(-Hc // 4), -(-Wc // 4)))
    z = h * np.repeat(np.repeat(lv, 4, axis=0), 4, axis=1)[:Hc, :Wc]
    return params, plane_depth(spec, params, z), rng.choice(np.asarray(ids), size=(Hc, Wc)).astype(np.int32)


def tie_frame(spec, rng, density, heading, x=0.0, y=0.0):
    """An untilted overhead pose and a constant depth buffer: principal = (0, 0, -1), right.z and up.z
    are exactly 0, so every point has the same z and only the tie rule decides a pixel."""
    h = height_for(spec, density)
    Hc, Wc = spec.height_px, spec.width_px
    db = np.full((Hc, Wc), depth_buffer(spec, 0.9 * h), dtype=np.float32)
    return look_down(x, y, h, heading), db, rng.choice(np.asarray(GENERIC_IDS), size=(Hc, Wc)).astype(np.int32)


def _case(name, spec, frames, envs=None, seg_ids=None, has=None, seq=None, nonfinite=False):
    ids0, has0 = default_ids()
    return Case(spec, np.asarray([f[0] for f in frames], dtype=np.float64).reshape(len(frames), 9),
                np.stack([f[1] for f in frames]).astype(np.float32), np.stack([f[2] for f in frames]).astype(np.int32),
                ids0 if seg_ids is None else seg_ids, has0 if has is None else has, name,
                list(range(len(frames))) if envs is None else list(envs), seq, nonfinite)


def _density(spec):
    """Camera pixels per map pixel (linear) that keep the footprint inside the map."""
    return max(2.0, spec.width_px / 200.0, spec.height_px / 160.0)


def _generic_case(name, Hc, Wc, n, seed):
    spec, rng = Spec(Hc, Wc), np.random.default_rng(seed)
    d = _density(spec)
    return _case(name, spec, [generic_frame(spec, rng, d, 0.3 + 0.4 * k, x=0.1 * k, y=-0.05 * k) for k in range(n)])


def _ties_case(name, Hc, Wc, seed):
    spec, rng = Spec(Hc, Wc), np.random.default_rng(seed)
    return _case(name, spec, [tie_frame(spec, rng, _density(spec), hd) for hd in (0.0, 0.3)])


def _big_case(name, seed):
    """All the 1023 x 1024 frames (the largest accepted frame, 512 chunks, k + 1 up to 2^20 - 2^10) in
    one launch: the boxes64 frame and the two tie frames."""
    spec, rng = Spec(1023, 1024), np.random.default_rng(seed)
    d = _density(spec)
    return _case(name, spec, [generic_frame(spec, rng, d, 0.3)] + [tie_frame(spec, rng, d, hd) for hd in (0.0, 0.3)])


def _zorder_case(name, Hc, Wc, seed):
    """near 500, far 1000: depth = 5e5 / (1000 - 500 db), so db = 2 is depth +inf, the float below 2
    depth 4e9 (a finite x / y beyond 2^31 map pixels), the float above 2 depth -2e9 (behind the camera).
    Frames 0 and 2 look down from 1 m (z = 1 - depth: above and below the floor, -inf), frame 1 looks up
    (z = 1 + depth, +inf).  Depths up to 9 m throw points past all four map edges.  A point of infinite
    depth has x, y in {+-inf, NaN} and lands on map pixel (0, 0), like a NaN one: frame 0 has NaN
    points there (NaN wins), frame 1 none (+inf wins), frame 2 none (-inf loses to the finite ones)."""
    spec, rng = Spec(Hc, Wc, near=500.0, far=1000.0), np.random.default_rng(seed)
    two = np.float32(2)
    special = [np.float32(np.inf), np.float32(-np.inf), two, np.nextafter(two, np.float32(0)), np.nextafter(two, np.float32(3))]
    frames = []
    for f in range(3):
        # a few depth levels, so that pixels share points of equal and of different z, of both signs
        dep = rng.choice(np.asarray([0.2, 0.5, 0.5, 0.9, 1.0, 1.25, 1.25, 2.0, 4.0, 9.0]), size=(Hc, Wc))
        db = depth_buffer(spec, dep)
        flat = db.reshape(-1)
        where = rng.choice(flat.size, size=8 * (len(special) + 1), replace=False)
        vals = special + ([np.float32(np.nan)] if f == 0 else [two])
        for k, w in enumerate(where):
            flat[w] = vals[k % len(vals)]
        if f == 0:  # the last NaN point (the winner of pixel (0, 0)) carries the sign bit: a key of raw bits would rank it lowest
            flat[np.nonzero(np.isnan(flat))[0][-1]] = -np.float32(np.nan)
        hd = 0.3 + f
        params = [0.2 * f - 0.2, 0.1 * f, 1.0, 0.2 * f - 0.15, 0.1 * f - 0.03, 0.0 if f != 1 else 2.0,
                  math.cos(hd), math.sin(hd), 0.0]
        frames.append((params, db, rng.choice(np.asarray(GENERIC_IDS), size=(Hc, Wc)).astype(np.int32)))
    return _case(name, spec, frames, nonfinite=True)


ID_SET = (INT32_MIN, -2, -1, 0, 1, 254, 255, 256, 300, INT32_MAX)
ID_IN = (-1, 0, 1, 254)                       # what the kernels' 256-entry table holds: -1 .. 254
ID_OUT = (INT32_MIN, -2, 255, 256, 300, INT32_MAX)
# env 0: everything overlaps on id 0 (1 + 2 + 3 + 4 = 10); env 1: no receptacle although its id (254)
# fills the frame, the obstacle range is all out of the table; env 2: 255 is obstacle, receptacle and cube (9)
IDS_RANGES = [dict(min_obstacle=-2, max_obstacle=1, receptacle=0, min_cube=0, max_cube=300),
              dict(min_obstacle=255, max_obstacle=INT32_MAX, receptacle=254, min_cube=1, max_cube=1),
              dict(min_obstacle=254, max_obstacle=255, receptacle=255, min_cube=255, max_cube=300)]
IDS_HAS = [1, 0, 1]
IDS_PLACED = [(-2, 300, 255), (INT32_MAX, 256, INT32_MIN), (255, 256, 300)]  # per env: its spans' out-of-range ids


def ids_split(npix):
    """First camera pixel of the half with out-of-range ids: a multiple of 512 (one wave's pixels)."""
    return -(-(npix // 2) // 512) * 512


def _ids_case(name, Hc, Wc, seed):
    """A sparse camera (every point on a map pixel of its own, so every code shows in the maps).  Camera
    pixels below ids_split(): ids -1 .. 254 only; from there on one out-of-range id per 512 pixels."""
    spec, rng = Spec(Hc, Wc), np.random.default_rng(seed)
    frames = []
    for e in range(3):
        params, db, _ = generic_frame(spec, rng, 0.45, 0.2 + 0.5 * e, levels=(0.0,))
        seg = rng.choice(np.asarray(ID_IN), size=Hc * Wc).astype(np.int32)
        for s, k0 in enumerate(range(ids_split(Hc * Wc), Hc * Wc, 512)):
            seg[k0 + int(rng.integers(0, min(512, Hc * Wc - k0)))] = IDS_PLACED[e][s % 3]
        frames.append((params, db, seg.reshape(Hc, Wc)))
    return _case(name, spec, frames, seg_ids=[dict(r) for r in IDS_RANGES], has=list(IDS_HAS))


def _modes_case(name, Hc, Wc, seed, dense, sparse):
    """Frame 0: a dense unrotated camera, every chunk's box of map pixels inside the LDS window;
    frame 1: (density, heading) = sparse, chunks whose boxes exceed it (hash mode)."""
    spec, rng = Spec(Hc, Wc), np.random.default_rng(seed)
    return _case(name, spec, [generic_frame(spec, rng, dense, 0.0, tilt=False),
                              generic_frame(spec, rng, sparse[0], sparse[1])])


def _order_case(name, Hc, Wc, seed):
    """Three frames onto env 0's slot, in list order; the earlier the frame, the higher its floor, so
    a key rule that let z outrank the frame order would keep the wrong frame.  One frame onto env 1's."""
    spec, rng = Spec(Hc, Wc), np.random.default_rng(seed)
    d = _density(spec)
    frames = [generic_frame(spec, rng, d, 0.3 + 0.1 * k, x=0.03 * k, levels=(lv, lv + 0.05)) for k, lv in enumerate((0.4, 0.2, 0.0))]
    frames.append(generic_frame(spec, rng, d, 1.0))
    return _case(name, spec, frames, envs=[0, 0, 0, 1], seq=[0, 1, 2, 0])


BUILDERS = collections.OrderedDict()
for _k, (_h, _w) in enumerate(((40, 67), (8, 312), (8, 313), (3, 1024))):
    BUILDERS['widths-%dx%d' % (_h, _w)] = functools.partial(_generic_case, Hc=_h, Wc=_w, n=1, seed=10 + _k)
# width 67 again, tall enough for a chunk that starts in a row's last column (chunk 37: 37 * 2048 % 67 = 66)
# and so reaches the row table's last entry, 31
BUILDERS['rows-1162x67'] = functools.partial(_generic_case, Hc=1162, Wc=67, n=1, seed=14)
# NP % 4 = 1, 3, 3 (one partial chunk only), 3, 2 (one partial chunk), 0 and 0 (no tail at all)
for _k, (_h, _w) in enumerate(((31, 311), (9, 1023), (9, 67), (7, 69), (6, 67), (16, 128), (8, 1024))):
    BUILDERS['unaligned-%dx%d' % (_h, _w)] = functools.partial(_generic_case, Hc=_h, Wc=_w, n=3, seed=20 + _k)
for _k, (_h, _w) in enumerate(((128, 1024), (130, 1024))):
    BUILDERS['boxes64-%dx%d' % (_h, _w)] = functools.partial(_generic_case, Hc=_h, Wc=_w, n=1, seed=30 + _k)
BUILDERS['boxes64+ties-1023x1024'] = functools.partial(_big_case, seed=33)
for _k, (_h, _w) in enumerate(((40, 67), (8, 313), (130, 1024))):
    BUILDERS['ties-%dx%d' % (_h, _w)] = functools.partial(_ties_case, Hc=_h, Wc=_w, seed=40 + _k)
for _k, (_h, _w) in enumerate(((40, 67), (8, 313))):
    BUILDERS['zorder-%dx%d' % (_h, _w)] = functools.partial(_zorder_case, Hc=_h, Wc=_w, seed=50 + _k)
    BUILDERS['ids-%dx%d' % (_h, _w)] = functools.partial(_ids_case, Hc=_h, Wc=_w, seed=60 + _k)
BUILDERS['modes-40x67'] = functools.partial(_modes_case, Hc=40, Wc=67, seed=70, dense=2.0, sparse=(0.45, 0.3))
BUILDERS['modes-8x640'] = functools.partial(_modes_case, Hc=8, Wc=640, seed=71, dense=4.0, sparse=(3.2, 0.5))
for _k, (_h, _w) in enumerate(((8, 313), (130, 1024))):
    BUILDERS['order-%dx%d' % (_h, _w)] = functools.partial(_order_case, Hc=_h, Wc=_w, seed=80 + _k)
CASE_IDS = list(BUILDERS)
TIE_FRAMES = {'ties-40x67': (0, 1), 'ties-8x313': (0, 1), 'ties-130x1024': (0, 1), 'boxes64+ties-1023x1024': (1, 2)}


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name](name)


# ---- the numpy model -----------------------------------------------------------------------------
def assert_host_cast():
    """The non-finite cases rely on numpy's float -> int32 cast of NaN, +-inf and values >= 2^31 being
    INT32_MIN (x86 cvttss2si), which np.clip then takes to pixel 0."""
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        got = np.float32([np.nan, np.inf, -np.inf, 3e9]).astype(np.int32)
    assert (got == INT32_MIN).all(), 'this host casts float32 [nan, inf, -inf, 3e9] to int32 as %s, not INT32_MIN: ' \
        'oracle.ingest cannot arbitrate the non-finite cases here' % got.tolist()


@contextlib.contextmanager
def quiet(nonfinite):
    """numpy's warnings of the non-finite cases (invalid value encountered in cast / multiply / ...)."""
    if nonfinite:
        assert_host_cast()
    with warnings.catch_warnings(), np.errstate(all='ignore' if nonfinite else 'warn'):
        if nonfinite:
            warnings.simplefilter('ignore', RuntimeWarning)
        yield


def points(spec, params, depth_buffer_):
    """Camera.capture_image's points [NP, 3] float32, op for op as oracle.ingest forms them."""
    FAR, NEAR = spec.far, spec.near
    Hc, Wc = depth_buffer_.shape
    depth = FAR * NEAR / (FAR - (FAR - NEAR) * depth_buffer_)
    camera_position = np.array(params[0:3], dtype=np.float32)
    principal = np.array(params[3:6], dtype=np.float32) - camera_position
    principal = principal / np.linalg.norm(principal)
    camera_up = np.array(params[6:9], dtype=np.float32)
    up = camera_up - np.dot(camera_up, principal) * principal
    up = up / np.linalg.norm(up)
    right = np.cross(principal, up)
    right = right / np.linalg.norm(right)
    pixel_x = spec.cx2 * (np.arange(Wc, dtype=np.float32) / Wc - 0.5)
    pixel_y = spec.cy2 * (0.5 - (np.arange(Hc, dtype=np.float32) + 1) / Hc)
    pixel_xv, pixel_yv = np.meshgrid(pixel_x, pixel_y)
    pts = camera_position + depth[:, :, np.newaxis] * (principal + pixel_xv[:, :, np.newaxis] * right
                                                       + pixel_yv[:, :, np.newaxis] * up)
    assert pts.dtype == np.float32
    return pts.reshape(-1, 3)


def codes(seg_raw, ids, has):
    """seg * 8 per body id: the reference's float sum of 1/8 multiples as the integer sum."""
    r = np.asarray(seg_raw).reshape(-1).astype(np.int64)
    c = (r == 0) * 1 + ((r >= ids['min_obstacle']) & (r <= ids['max_obstacle'])) * 2
    c = c + ((r == ids['receptacle']) * 3 if has else 0)
    return (c + ((r >= ids['min_cube']) & (r <= ids['max_cube'])) * 4).astype(np.int64)


def zkeys(z):
    """float32 z -> uint32, monotone in z, NaN (of either sign) above everything."""
    b = np.ascontiguousarray(z, dtype=np.float32).view(np.uint32)
    zk = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))
    return np.where(np.isnan(z), np.uint32(0xffffffff), zk).astype(np.uint32)


def frame_model(case_, n, H, W):
    """Frame n's points as the kernels see them: map pixel, code, z key, and the per-chunk boxes
    (i0, i1, j0, j1) of 2048 consecutive camera pixels."""
    with quiet(case_.nonfinite):
        pts = points(case_.spec, case_.cam_params[n], case_.depth[n])
        pi = np.clip(np.floor(H / 2 - pts[:, 1] * PPM).astype(np.int32), 0, H - 1)
        pj = np.clip(np.floor(W / 2 + pts[:, 0] * PPM).astype(np.int32), 0, W - 1)
    e = case_.envs[n]
    boxes = np.array([[pi[k:k + PTS].min(), pi[k:k + PTS].max() + 1, pj[k:k + PTS].min(), pj[k:k + PTS].max() + 1]
                      for k in range(0, len(pi), PTS)], dtype=np.int64)
    return FrameRef(pi.astype(np.int64), pj.astype(np.int64), codes(case_.seg_raw[n], case_.seg_ids[e], case_.has_receptacle[e]),
                    zkeys(pts[:, 2]), boxes)


def frame_order(case_, seq=None):
    """Frame indices in the order the launch applies them (frames of one slot by seq; stable)."""
    seq = case_.seq if seq is None else seq
    return list(range(len(case_.envs))) if seq is None else sorted(range(len(case_.envs)), key=lambda n: seq[n])


def reference(ov, oc, case_, seq=None):
    """oracle.ingest of every frame, in launch order, in place on ov / oc [E, H, W] (env e: the slot
    of robot AGENT of env e).  Returns the model's view of the same launch: per frame the FrameRef and
    chunk boxes, per env and map pixel the winning frame (-1: untouched), camera pixel and code."""
    E, H, W = ov.shape
    frames = [frame_model(case_, n, H, W) for n in range(len(case_.envs))]
    win_frame = np.full((E, H * W), -1, dtype=np.int64)
    win_k = np.full((E, H * W), -1, dtype=np.int64)
    win_code = np.zeros((E, H * W), dtype=np.int64)
    for n in frame_order(case_, seq):
        e, f = case_.envs[n], frames[n]
        with quiet(case_.nonfinite):
            O.ingest(ov[e], oc[e], case_.depth[n], case_.seg_raw[n], list(case_.cam_params[n]), case_.spec, case_.seg_ids[e],
                     bool(case_.has_receptacle[e]))
        cell = f.pi * W + f.pj
        score = np.zeros(H * W, dtype=np.uint64)        # (zkey, k + 1) per point, max per cell
        np.maximum.at(score, cell, (f.zk.astype(np.uint64) << np.uint64(20)) | (np.arange(len(cell), dtype=np.uint64) + np.uint64(1)))
        hit = score != 0
        k = (score[hit] & np.uint64(0xfffff)).astype(np.int64) - 1
        win_frame[e, hit], win_k[e, hit], win_code[e, hit] = n, k, f.code[k]
    shp = (E, H, W)
    return Ref(frames, [f.boxes for f in frames], win_frame.reshape(shp), win_k.reshape(shp), win_code.reshape(shp))


def model_maps(ov, oc, case_, ref):
    """What the key rule alone leaves in the maps: in place on ov / oc [E, H, W]."""
    hit = ref.win_frame >= 0
    ov[hit] = (ref.win_code[hit].astype(np.float32) * np.float32(0.125))
    for n, f in enumerate(ref.frames):
        obst = f.code == 2
        oc[case_.envs[n]][f.pi[obst], f.pj[obst]] = 1


def model_keys(case_, ref, tag0, seq=None):
    """The key map [E, H, W] uint64 of a launch with base tag tag0 on touched pixels (0 elsewhere) and
    the mask of touched pixels."""
    seq = case_.seq if seq is None else seq
    hit = ref.win_frame >= 0
    keys = np.zeros(ref.win_frame.shape, dtype=np.uint64)
    n = ref.win_frame[hit]
    tag = tag0 + (np.asarray(seq, dtype=np.int64)[n] if seq is not None else np.zeros(len(n), dtype=np.int64))
    zk = np.empty(len(n), dtype=np.uint64)
    for f in np.unique(n):
        zk[n == f] = ref.frames[f].zk[ref.win_k[hit][n == f]]
    keys[hit] = ((tag.astype(np.uint64) << np.uint64(56)) | (zk << np.uint64(24))
                 | ((ref.win_k[hit] + 1).astype(np.uint64) << np.uint64(4)) | ref.win_code[hit].astype(np.uint64))
    return keys, hit


@functools.lru_cache(maxsize=None)
def solved(name, reverse=False):
    """(case, oracle overhead, oracle occupancy, Ref) of a case from the scenes' own maps, computed once
    per process and shared read-only.  reverse: the three frames of the order cases' first slot in
    reversed order."""
    c = case(name)
    seq = None
    if reverse:
        top = max(c.seq)
        seq = [top - s if e == c.envs[0] else s for s, e in zip(c.seq, c.envs)]
    ov, oc = start_maps()
    ref = reference(ov, oc, c, seq)
    for a in (ov, oc):
        a.setflags(write=False)
    return c, ov, oc, ref, seq
