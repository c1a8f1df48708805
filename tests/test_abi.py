"""CPU: libsimaps.so loads, exports every symbol include/simaps.h declares, host helpers work.

No kernel is launched here (no GPU in the CPU tier)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'simaps.h')


def declared_symbols():
    txt = open(HEADER).read()
    return sorted(set(re.findall(r'\b(simaps_[a-z_0-9]+)\s*\(', txt)))


def test_header_declares_the_abi():
    assert declared_symbols() == sorted(['simaps_abi_version', 'simaps_last_error', 'simaps_fault_status',
                                         'simaps_num_channels', 'simaps_sp_distance', 'simaps_shortest_path',
                                         'simaps_ingest', 'simaps_ingest_chunks', 'simaps_path_mode', 'simaps_robot_mask', 'simaps_pack_robots',
                                         'simaps_get_state', 'simaps_sssp_grid',
                                         'simaps_grid_path', 'simaps_rec_cache_bytes', 'simaps_sp_lookup',
                                         'simaps_get_state_mixed', 'simaps_source_hash', 'simaps_occupancy_scatter',
                                         'simaps_build_cspace', 'simaps_snap_sources', 'simaps_global_maps'])


def test_library_exports_every_declared_symbol():
    from simaps import _lib
    for name in declared_symbols():
        assert hasattr(_lib.lib, name), name
        assert isinstance(getattr(_lib.lib, name), ctypes._CFuncPtr)
    assert set(_lib.EXPORTED) == set(declared_symbols())
    assert _lib.lib.simaps_abi_version() == 8


def test_struct_layouts_match_header():
    from simaps import _lib
    assert _lib.ROBOT_DTYPE.itemsize == 72
    assert _lib.ENV_DTYPE.itemsize == 32
    assert _lib.AGENT_DTYPE.itemsize == 12
    assert ctypes.sizeof(_lib.Config) == 18 * 4 + 4 * 8
    assert ctypes.sizeof(_lib.Debug) == 5 * 8


def test_rec_cache_record_size():
    """simaps_rec_cache_bytes: a 16-byte header and the room rect's (h + 2) x ((w + 2) | 1) float32
    distance array, rounded up to 256 bytes; refuses a bad config (host-side only)."""
    from simaps import _lib, batch, synthetic
    for name in ('lifting_4-small_divider', 'pushing_4-large_empty'):
        s = synthetic.make_scene(name, 0)
        c = batch.make_config(s['flags'], s['room_width'], s['room_length'])
        want = (16 + (c.room_h + 2) * ((c.room_w + 2) | 1) * 4 + 255) // 256 * 256
        assert _lib.lib.simaps_rec_cache_bytes(c) == want
    c.room_h = 0
    assert _lib.lib.simaps_rec_cache_bytes(c) == _lib.EINVAL
    assert _lib.lib.simaps_sp_lookup(None, 1, None, None, None, 1, None, None) == _lib.EINVAL


def test_host_robot_masks_match_reference():
    """simaps_robot_mask (host C++) == Mapper._create_robot_mask goldens (envs.py:2218-2242)."""
    from simaps import _lib
    import goldens as G
    g = G.load('masks.npz')
    for t in ('lifting_robot', 'pushing_robot', 'throwing_robot', 'rescue_robot'):
        assert np.array_equal(_lib.robot_mask(t), g[t]), t
    assert np.array_equal(_lib.robot_mask('lifting_robot', True), g['lifting_robot_with_cube'])


@pytest.mark.parametrize('cfg_name', ['lifting_1-small_empty', 'lifting_4-small_divider', 'rescue_4-small_empty',
                                      'lifting_4-large_empty-nonspatial', 'lifting_2_pushing_2-large_empty-all'])
def test_num_channels(cfg_name):
    from simaps import _lib, batch, synthetic
    flags = synthetic.config_flags(cfg_name)
    cfg = synthetic.CONFIGS[cfg_name]
    nr = sum(sum(g.values()) for g in cfg['robot_config'])
    c = batch.make_config(flags, 0.5 if cfg['env_name'].startswith('small') else 1.0, 1.0)
    assert _lib.lib.simaps_num_channels(c, nr) == synthetic.num_channels(flags, nr)


def test_error_paths_do_not_launch():
    from simaps import _lib, batch, synthetic
    flags = synthetic.config_flags('lifting_4-small_divider')
    c = batch.make_config(flags, 0.5, 1.0)
    assert _lib.lib.simaps_get_state(c, 0, None, None, None, None, None, None, None, 0, None, None) == 0
    c.intention_map_line_thickness = 5
    rc = _lib.lib.simaps_get_state(c, 1, None, None, None, None, None, None, None, 0, None, None)
    assert rc == -2 and b'thickness' in _lib.lib.simaps_last_error()
    assert _lib.lib.simaps_sssp_grid(1, 300, 300, None, None, None, 0, 0, 300, 300, None) == -1
    assert _lib.lib.simaps_grid_path(1, 30, 30, None, None, None, 0, 0, 30, 30, 0, None, None, None) == -1
    assert _lib.lib.simaps_grid_path(0, 30, 30, None, None, None, 0, 0, 30, 30, 8, None, None, None) == 0


def test_fault_status_without_gpu():
    """The host-mapped fault word needs a device: without one the call reports SIMAPS_EHIP
    instead of crashing; with one the word starts clear."""
    from simaps import _lib
    rc = _lib.lib.simaps_fault_status(0)
    assert rc in (0, _lib.EHIP)


def test_statebatch_refuses_cpu_device():
    """The product path has no CPU fallback: a host device is refused before any launch."""
    from simaps import batch, synthetic
    with pytest.raises(ValueError):
        batch.StateBatch([synthetic.make_scene('lifting_1-small_empty', 0)], device='cpu')


def test_ingest_chunk_count_and_argument_checks():
    """simaps_ingest_chunks sizes the boxes scratch (one entry per 2048 camera pixels); simaps_ingest
    refuses bad cameras, NULL buffers, unsupported widths and epochs outside [0, 255] before any launch."""
    import ctypes
    from simaps import _lib, batch, camera, synthetic
    L = _lib.lib
    for h, w in ((156, 277), (156, 156), (1, 1), (64, 32)):
        assert L.simaps_ingest_chunks(h, w) == -(-h * w // 2048)
    assert L.simaps_ingest_chunks(0, 277) == _lib.EINVAL
    c = batch.make_config(synthetic.config_flags('lifting_4-small_divider'), 0.5, 1.0)
    spec = camera.CAMERAS['forward']
    cam = _lib.Camera(spec.height_px, spec.width_px, spec.near, spec.far, spec.cx2, spec.cy2)
    assert L.simaps_ingest(c, cam, 0, *([None] * 9), 1, None) == 0                  # nothing to do
    assert L.simaps_ingest(c, cam, 1, *([None] * 9), 1, None) == _lib.EINVAL        # NULL buffers
    bad = _lib.Camera(spec.height_px, spec.width_px, spec.far, spec.near, spec.cx2, spec.cy2)
    assert L.simaps_ingest(c, bad, 1, *([None] * 9), 1, None) == _lib.EINVAL        # near >= far
    p = ctypes.c_void_p(8)  # never dereferenced: the width check comes first
    wide = _lib.Camera(8, 2000, spec.near, spec.far, spec.cx2, spec.cy2)
    assert L.simaps_ingest(c, wide, 1, *([p] * 9), 1, None) == _lib.EUNSUPPORTED
    for epoch in (-1, 256):  # the key map's launch epoch: 0 (zeroing mode) .. 255; refused before any launch
        assert L.simaps_ingest(c, cam, 1, *([p] * 9), epoch, None) == _lib.EINVAL


def test_path_mode_setter():
    """simaps_path_mode returns the previous mode, accepts 0 (automatic), 1 (compact), 2 (early
    exit) and 3 (early exit, sweeps overlapped) and refuses anything else without changing the mode
    (host-side only)."""
    from simaps import _lib
    L = _lib.lib
    prev = L.simaps_path_mode(1)
    try:
        assert L.simaps_path_mode(2) == 1
        assert L.simaps_path_mode(3) == 2
        assert L.simaps_path_mode(0) == 3
        for bad in (-1, 4):
            assert L.simaps_path_mode(bad) == _lib.EINVAL
        assert L.simaps_path_mode(0) == 0  # unchanged by the refused calls
    finally:
        L.simaps_path_mode(prev)


def test_gridgraph_window_limits_match_header():
    """The drop-in GridGraph's `large` flag (the global-memory kernels of csrc/grid_large.h) follows the
    LDS window limits of include/simaps.h (SIMAPS_MAX_ROOM_CELLS / SIMAPS_MAX_ROOM_W) with the same
    rule the ABI applies when it picks the kernels."""
    from simaps import vector_env
    txt = open(HEADER).read()
    cells = int(re.search(r'#define SIMAPS_MAX_ROOM_CELLS (\d+)', txt).group(1))
    maxw = int(re.search(r'#define SIMAPS_MAX_ROOM_W (\d+)', txt).group(1))
    assert (vector_env.MAX_WINDOW_CELLS, vector_env.MAX_WINDOW_W) == (cells, maxw)
    fits = vector_env.window_fits
    assert fits(44, 92) and fits(92, 92) and fits(1, 1)            # small / large rooms, one cell
    assert not fits(93, 93) and not fits(40, 121) and not fits(0, 5)
    for h in range(1, 200, 7):
        for w in range(1, 130, 3):
            assert fits(h, w) == (w <= maxw and (h + 2) * ((w + 2) | 1) <= cells)


def test_library_source_hash_matches_the_tree():
    """simaps_source_hash: the library carries the hash of the sources it was
    built from, and it is this tree's (else simaps._lib would have refused to load it)."""
    from simaps import _lib, _srchash
    _lib.lib.simaps_source_hash.restype = ctypes.c_char_p
    assert _lib.lib.simaps_source_hash().decode() == _srchash.source_hash()
    rels = [r for r, _ in _srchash.source_files()]
    assert 'include/simaps.h' in rels and 'csrc/simaps.hip' in rels and 'csrc/grid_large.h' in rels


def test_build_switches_are_the_makefile_table():
    """Every SIMAPS_* macro that the device sources test in a preprocessor condition is an ABI constant
    (defined unconditionally in csrc/ or include/), a unit-mode macro that an including unit sets for
    itself, or a build switch named in the table at the top of csrc/Makefile -- and the table names no
    other.  A new experiment's switch has to enter the table, and leave it with its code."""
    import glob
    csrc = os.path.join(ROOT, 'spatial-intention-maps_amd', 'csrc')
    srcs = sorted(f for ext in ('hip', 'h', 'inc') for f in glob.glob(os.path.join(csrc, '*.' + ext)))
    assert len(srcs) > 30
    tested, unconditional = set(), set()
    for path in srcs + sorted(glob.glob(os.path.join(ROOT, 'include', '*.h'))):
        text = open(path).read().replace('\\\n', ' ')
        guard = re.search(r'^#ifndef (\w+)\n#define \1\n', text, re.M)  # a header's include guard is no condition
        open_ifs = []  # the conditions a line stands under, innermost last
        for line in text.splitlines():
            code = line.split('//')[0]
            m = re.match(r'\s*#\s*(\w+)\s*(.*)', code)
            if m and m.group(1) in ('if', 'ifdef', 'ifndef', 'elif'):
                if path in srcs:
                    tested |= set(re.findall(r'\bSIMAPS_\w+', m.group(2)))
                if m.group(1) != 'elif':
                    open_ifs.append(bool(guard) and m.group(1) == 'ifndef' and m.group(2).strip() == guard.group(1))
            elif m and m.group(1) == 'endif':
                open_ifs.pop()
            elif m and m.group(1) == 'define' and all(open_ifs):
                unconditional.add(m.group(2).split('(')[0].split()[0])
        assert not open_ifs, path
    unit_mode = {'SIMAPS_DEVICE_ONLY', 'SIMAPS_STATE16', 'SIMAPS_STORE_DTYPE'}
    switches = tested - unconditional - unit_mode
    top = []  # the Makefile's leading comment
    for line in open(os.path.join(csrc, 'Makefile')):
        if not line.startswith('#'):
            break
        top.append(line)
    table = set(re.findall(r'^#   (SIMAPS_\w+) ', ''.join(top), re.M))
    assert len(table) >= 8, table
    assert switches == table, (sorted(switches - table), sorted(table - switches))


def test_stale_library_is_refused(tmp_path):
    """A copy of the tree whose kernel source differs from what its libsimaps.so was built from -- here
    only a comment -- refuses to load the library; the unmodified copy loads it."""
    import shutil
    import subprocess
    import sys
    pkg = os.path.join(ROOT, 'spatial-intention-maps_amd')
    dst = tmp_path / 'repo'
    shutil.copytree(os.path.join(pkg, 'simaps'), dst / 'spatial-intention-maps_amd' / 'simaps',
                    ignore=shutil.ignore_patterns('__pycache__', 'libsimaps_*.so'))
    shutil.copytree(os.path.join(pkg, 'csrc'), dst / 'spatial-intention-maps_amd' / 'csrc')
    shutil.copytree(os.path.join(ROOT, 'include'), dst / 'include')
    code = 'import sys; sys.path.insert(0, %r); import simaps._lib' % str(dst / 'spatial-intention-maps_amd')
    env = {k: v for k, v in os.environ.items() if not k.startswith('SIMAPS_')}
    ok = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, env=env, timeout=300)
    assert ok.returncode == 0, ok.stderr
    src = dst / 'spatial-intention-maps_amd' / 'csrc' / 'simaps.hip'
    src.write_text(src.read_text().replace('// simaps.hip --', '// simaps.hip (edited) --', 1))
    bad = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, env=env, timeout=300)
    assert bad.returncode != 0
    assert 'StaleLibraryError' in bad.stderr and 'stale binary' in bad.stderr


def test_occupancy_map_host_side():
    """The OccupancyMap drop-in: no CPU path (the grid and every derived map live on the device),
    an unknown robot type refused; the host pixel-index helper equals the
    oracle's Mapper.position_to_pixel_indices (envs.py:2391-2397) on random and pixel-edge positions;
    the three OccupancyMap entries refuse bad arguments before any launch."""
    import oracle as O
    from simaps import _lib, batch, constants as K, synthetic, vector_env
    with pytest.raises(ValueError):
        vector_env.OccupancyMap('lifting_robot', 1.0, 0.5, device='cpu')
    with pytest.raises(ValueError):
        vector_env.OccupancyMap('lifting_robot', 1.0, 0.5, show_map=True, device='cpu')
    with pytest.raises(ValueError):
        vector_env.OccupancyMap('flying_robot', 1.0, 0.5)
    rs = np.random.RandomState(3)
    for _ in range(5000):
        x, y = rs.uniform(-1.5, 1.5, 2)
        if rs.rand() < 0.3:
            x, y = round(x * 96) / 96, round(y * 96) / 96
        want = O.position_to_pixel_indices(x, y, (184, 232))
        assert K.position_to_pixel_indices(x, y, (184, 232)) == (int(want[0]), int(want[1]))
    c = batch.make_config(synthetic.config_flags('lifting_4-small_divider'), 0.5, 1.0)
    L = _lib.lib
    assert L.simaps_build_cspace(c, 1, None, None, None, None, None, None, None) == _lib.EINVAL   # nothing asked
    assert L.simaps_build_cspace(c, 0, None, None, None, None, ctypes.c_void_p(8), None, None) == 0
    assert L.simaps_snap_sources(c, 1, None, None, None, None, None, 3, None, None) == _lib.EINVAL
    assert L.simaps_snap_sources(c, 1, None, None, None, None, None, 0, None, None) == 0
    assert L.simaps_occupancy_scatter(c, 1, None, None, None, 5, 0.25, None, None) == _lib.EINVAL
    assert L.simaps_occupancy_scatter(c, 2, None, None, None, 0, 0.25, None, None) == 0


def test_figure_channel_names_cover_the_state():
    """simaps.figures names every state channel in envs.py:2071-2113 order: as many names as
    simaps_num_channels gives channels, for every synthetic configuration."""
    from simaps import figures, synthetic
    for name, cfg in synthetic.CONFIGS.items():
        flags = synthetic.config_flags(name)
        nr = sum(sum(g.values()) for g in cfg['robot_config'])
        assert len(figures.channel_names(flags, nr)) == synthetic.num_channels(flags, nr), name
    img = np.array([[0.0, 0.5, 1.0, 1.33]], dtype=np.float32)
    assert figures.to_uint8_image(img).tolist() == [[0, 128, 255, 83]]  # (utils.to_uint8_image's uint8 wrap)
