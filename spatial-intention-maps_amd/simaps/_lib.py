"""ctypes binding of libsimaps.so (the C ABI declared in include/simaps.h, include/simaps_ctx.h,
include/simaps_action.h, include/simaps_state16.h, include/simaps_store.h, include/simaps_spec.h, include/simaps_spec_room.h,
include/simaps_spec_store.h, include/simaps_state_cache.h, include/simaps_state_cache_store.h, include/simaps_ingest_seq.h and include/simaps_action_as.h).

torch is imported FIRST so that libsimaps.so binds to the HIP runtime torch already loaded
(both resolve SONAME libamdhip64.so.7): one runtime instance, so torch device pointers and
streams are valid in our launches.  There is no CPU fallback: if the library is missing this
module raises at import.
"""
import ctypes
import os

import numpy as np
import torch  # noqa: F401  (must precede the CDLL load, see module docstring)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('SIMAPS_LIB', os.path.join(HERE, 'libsimaps.so'))

LIFTING, PUSHING, THROWING, RESCUE = 0, 1, 2, 3
TYPE_IDS = {'lifting_robot': LIFTING, 'pushing_robot': PUSHING, 'throwing_robot': THROWING, 'rescue_robot': RESCUE}
ENC_IDS = {'ramp': 0, 'binary': 1, 'line': 2, 'circle': 3}
ROT_IDS = {'fma': 0, 'plain': 1}  # SIMAPS_ROT_* (include/simaps.h)
MAX_ROBOTS = 8
MAX_PATH = 16

# numpy mirrors of the device structs (include/simaps.h), packed C layout
ROBOT_DTYPE = np.dtype([('x', '<f8'), ('y', '<f8'), ('heading', '<f8'), ('target_x', '<f8'), ('target_y', '<f8'),
                        ('type', '<i4'), ('group_index', '<i4'), ('lifting', '<i4'), ('idle', '<i4'),
                        ('intention_off', '<i4'), ('intention_len', '<i4'), ('history_off', '<i4'),
                        ('history_len', '<i4')], align=True)
ENV_DTYPE = np.dtype([('receptacle_x', '<f8'), ('receptacle_y', '<f8'), ('has_receptacle', '<i4'),
                      ('robot_off', '<i4'), ('num_robots', '<i4'), ('reserved', '<i4')], align=True)
ABI_VERSION = 8  # include/simaps.h SIMAPS_ABI_VERSION
ACTION_ABI_VERSION = 1  # include/simaps_action.h SIMAPS_ACTION_ABI_VERSION
STATE16_ABI_VERSION = 1  # include/simaps_state16.h SIMAPS_STATE16_ABI_VERSION
STORE_ABI_VERSION = 1  # include/simaps_store.h SIMAPS_STORE_ABI_VERSION
MAX_MIXED = 8  # SIMAPS_MAX_MIXED
AGENT_DTYPE = np.dtype([('env', '<i4'), ('robot', '<i4'), ('map_slot', '<i4')], align=True)
assert ROBOT_DTYPE.itemsize == 72 and ENV_DTYPE.itemsize == 32 and AGENT_DTYPE.itemsize == 12


SEG_IDS_DTYPE = np.dtype([('min_obstacle', '<i4'), ('max_obstacle', '<i4'), ('receptacle', '<i4'),
                          ('min_cube', '<i4'), ('max_cube', '<i4'), ('has_receptacle', '<i4')], align=True)


class Camera(ctypes.Structure):
    """simaps_camera (include/simaps.h)."""
    _fields_ = [('height_px', ctypes.c_int32), ('width_px', ctypes.c_int32), ('near_m', ctypes.c_double),
                ('far_m', ctypes.c_double), ('cx2', ctypes.c_double), ('cy2', ctypes.c_double)]


class Config(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in (
        'H', 'W', 'room_i0', 'room_j0', 'room_h', 'room_w', 'use_robot_map', 'use_distance_to_receptacle_map',
        'use_shortest_path_to_receptacle_map', 'use_shortest_path_map', 'use_intention_map',
        'intention_map_encoding', 'intention_map_line_thickness', 'use_history_map', 'use_intention_channels',
        'intention_channel_spatial', 'layout_chw', 'rotate_rounding')] + \
        [(n, ctypes.c_double) for n in ('distance_to_receptacle_map_scale', 'shortest_path_map_scale',
                                         'intention_map_scale', 'intention_channel_nonspatial_scale')]


class Debug(ctypes.Structure):
    """simaps_debug: optional per-agent outputs (parity tests) and the receptacle distance cache."""
    _fields_ = [('cspace', ctypes.c_void_p), ('sources', ctypes.c_void_p), ('dist', ctypes.c_void_p),
                ('status', ctypes.c_void_p), ('rec_cache', ctypes.c_void_p)]


class SimapsError(RuntimeError):
    pass


class StaleLibraryError(ImportError):
    """libsimaps.so was built from sources other than the tree's (simaps_source_hash)."""


def _check_source_hash(L, path):
    """Refuse a library built from other sources than this tree's csrc/ + include/ (a stale .so left
    over from before a kernel edit would otherwise run silently, on the GPU box too).  An A/B
    timing of another revision's build names the hash it expects in SIMAPS_AB_SOURCE_HASH."""
    from . import _srchash
    if not hasattr(L, 'simaps_source_hash'):
        if os.environ.get('SIMAPS_AB_OLD_ABI'):  # (an older revision's A/B build predates the export)
            return
        raise StaleLibraryError('%s has no simaps_source_hash: built before the stale-binary guard; rebuild it with '
                                '`make -C spatial-intention-maps_amd/csrc`' % path)
    L.simaps_source_hash.restype = ctypes.c_char_p
    built = L.simaps_source_hash().decode()
    want = os.environ.get('SIMAPS_AB_SOURCE_HASH') or _srchash.source_hash()
    if built != want:
        raise StaleLibraryError('%s was built from other sources (hash %s) than this tree\'s (%s): a stale binary -- '
                                'rebuild it with `make -C spatial-intention-maps_amd/csrc` (and `... diag` for the '
                                'diagnostic builds)' % (path, built[:16], want[:16]))


# include/simaps_ctx.h: the context functions, and the compute entry points that have a twin
# simaps_ctx_<name> taking the context first
CTX_MANAGEMENT = ('simaps_ctx_create', 'simaps_ctx_destroy', 'simaps_ctx_device', 'simaps_ctx_fault_status',
                  'simaps_ctx_fault_info', 'simaps_ctx_path_mode')
CTX_TWINS = ('get_state', 'get_state_mixed', 'sp_distance', 'sp_lookup', 'shortest_path', 'ingest', 'sssp_grid',
             'grid_path', 'occupancy_scatter', 'build_cspace', 'snap_sources', 'global_maps')
EXPORTED_CTX = CTX_MANAGEMENT + tuple('simaps_ctx_' + n for n in CTX_TWINS)

# SIMAPS_K_* (include/simaps_ctx.h): kernel id of a fault record's `where` word -> kernel name
# include/simaps_action.h: the step back from the policy (its compute entry point has a context twin too)
EXPORTED_ACTION = ('simaps_action_abi_version', 'simaps_num_output_channels', 'simaps_store_new_action',
                   'simaps_ctx_store_new_action')
ACTION_SHORTEST_PATH, ACTION_WRITE_BACK = 1, 2  # SIMAPS_ACTION_* flag bits

# include/simaps_state16.h: the state stack rendered as bf16 / fp16 (with its context twin)
EXPORTED_STATE16 = ('simaps_state16_abi_version', 'simaps_get_state_as', 'simaps_ctx_get_state_as')
STATE_F32, STATE_BF16, STATE_F16 = 0, 1, 2  # SIMAPS_STATE_*
STATE_DTYPES = {torch.float32: STATE_F32, torch.bfloat16: STATE_BF16, torch.float16: STATE_F16}


def state_dtype_id(dtype):
    """SIMAPS_STATE_* of a torch dtype; ValueError for any other than float32, bfloat16, float16."""
    try:
        return STATE_DTYPES[dtype]
    except (KeyError, TypeError):
        raise ValueError('state dtype %r: torch.float32, torch.bfloat16 or torch.float16' % (dtype,)) from None


# include/simaps_store.h: states rendered into a caller-owned store at device-chosen rows, and the
# mixed launch in bf16 / fp16 (each with its context twin)
EXPORTED_STORE = ('simaps_store_abi_version', 'simaps_get_state_into', 'simaps_ctx_get_state_into',
                  'simaps_get_state_mixed_as', 'simaps_ctx_get_state_mixed_as')


# include/simaps_spec.h: which get_state kernel a call takes (host-only query)
EXPORTED_SPEC = ('simaps_spec_abi_version', 'simaps_get_state_instance')
SPEC_ABI_VERSION = 1  # SIMAPS_SPEC_ABI_VERSION
SPEC_GENERIC, SPEC_S1, SPEC_S2 = 0, 1, 2  # SIMAPS_SPEC_*
SPEC_NAMES = {SPEC_GENERIC: 'generic', SPEC_S1: 'S1', SPEC_S2: 'S2'}

# include/simaps_spec_room.h: the room class of the instance a get_state call takes (host-only query)
EXPORTED_SPEC_ROOM = ('simaps_spec_room_abi_version', 'simaps_get_state_room_class')
SPEC_ROOM_ABI_VERSION = 1  # SIMAPS_SPEC_ROOM_ABI_VERSION
ROOM_NONE, ROOM_SMALL = 0, 1  # SIMAPS_ROOM_*
ROOM_NAMES = {ROOM_NONE: 'none', ROOM_SMALL: 'small'}
ROOM_SMALL_SHAPE = (184, 232, 44, 92)  # SIMAPS_ROOM_SMALL_H / _W / _RH / _RW

# include/simaps_spec_store.h: the same two answers for the store launches and the 16-bit launches
EXPORTED_SPEC_STORE = ('simaps_spec_store_abi_version', 'simaps_get_state_instance_as',
                       'simaps_get_state_room_class_as')
SPEC_STORE_ABI_VERSION = 1  # SIMAPS_SPEC_STORE_ABI_VERSION


# include/simaps_state_cache.h: get_state with a per-map-slot record of what an unchanged map makes (with
# its context twin)
EXPORTED_STATE_CACHE = ('simaps_state_cache_abi_version', 'simaps_state_cache_bytes', 'simaps_get_state_cached',
                        'simaps_ctx_get_state_cached')
STATE_CACHE_ABI_VERSION = 1  # SIMAPS_STATE_CACHE_ABI_VERSION
STATE_CACHE_MAGIC = 0x53433031  # SIMAPS_STATE_CACHE_MAGIC
# simaps_state_cache_header: the head of one record
STATE_CACHE_HEADER_DTYPE = np.dtype([(n, '<i4') for n in (
    'magic', 'H', 'W', 'room_i0', 'room_j0', 'room_h', 'room_w', 'cspace_radius', 'has_receptacle', 'rec_i', 'rec_j',
    'reserved0', 'snap_i', 'snap_j', 'src_ok')] + [('dist_max', '<f4'), ('hits', '<u4'), ('misses', '<u4'),
                                                    ('reserved1', '<u4', (2,))], align=True)
assert STATE_CACHE_HEADER_DTYPE.itemsize == 80

# include/simaps_state_cache_store.h: the same cache for the store launches and the 16-bit launches (each
# with its context twin), and the host-only query of which calls use it
EXPORTED_STATE_CACHE_STORE = ('simaps_state_cache_store_abi_version', 'simaps_state_cache_applies',
                              'simaps_get_state_into_cached', 'simaps_ctx_get_state_into_cached',
                              'simaps_get_state_as_cached', 'simaps_ctx_get_state_as_cached')
STATE_CACHE_STORE_ABI_VERSION = 1  # SIMAPS_STATE_CACHE_STORE_ABI_VERSION


# include/simaps_ingest_seq.h: several frames per map slot in one launch, applied in order (with its
# context twin)
EXPORTED_INGEST_SEQ = ('simaps_ingest_seq_abi_version', 'simaps_ingest_seq', 'simaps_ctx_ingest_seq')
INGEST_SEQ_ABI_VERSION = 1  # SIMAPS_INGEST_SEQ_ABI_VERSION
MAX_SEQ = 255  # frames of one map slot per launch: the key's 8-bit tag, 0 being "no key"


# include/simaps_action_as.h: the action call for 16-bit Q maps, with the exploration draw on the device
# (with its context twin)
EXPORTED_ACTION_AS = ('simaps_action_as_abi_version', 'simaps_store_new_action_as', 'simaps_ctx_store_new_action_as')
ACTION_AS_ABI_VERSION = 1  # SIMAPS_ACTION_AS_ABI_VERSION


K_NAMES = {1: 'get_state', 2: 'get_state_mixed', 3: 'sp_distance', 4: 'path', 5: 'sssp_grid', 6: 'grid_path',
           7: 'gl_sssp', 8: 'gl_tile', 9: 'gl_path', 10: 'occupancy_map', 11: 'global_maps', 12: 'action',
           13: 'get_state_into'}


def _load(path=LIB_PATH):
    """Bind the C ABI of the library at `path` (the product libsimaps.so by default; tests also load
    diagnostic builds of the same ABI through this)."""
    if not os.path.exists(path):
        raise ImportError('libsimaps.so not found at %s -- build it with `make -C spatial-intention-maps_amd/csrc` '
                          '(or __graft_entry__.build()); there is no CPU fallback' % path)
    L = ctypes.CDLL(path)
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    L.simaps_abi_version.restype = i32
    _check_source_hash(L, path)
    L.simaps_last_error.restype = ctypes.c_char_p
    L.simaps_num_channels.argtypes = [ctypes.POINTER(Config), i32]
    L.simaps_num_channels.restype = i32
    L.simaps_pack_robots.argtypes = [i32, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp]
    L.simaps_pack_robots.restype = i32
    L.simaps_robot_mask.argtypes = [i32, i32, vp]
    L.simaps_robot_mask.restype = i32
    L.simaps_get_state.argtypes = [ctypes.POINTER(Config), i32, vp, vp, vp, vp, vp, vp, vp, i32,
                                   ctypes.POINTER(Debug), vp]
    L.simaps_get_state.restype = i32
    if hasattr(L, 'simaps_get_state_mixed'):  # (ABI 8; absent only in an older revision's A/B build)
        L.simaps_get_state_mixed.argtypes = [ctypes.POINTER(Config), vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                             vp, vp]
        L.simaps_get_state_mixed.restype = i32
    L.simaps_sp_distance.argtypes = [ctypes.POINTER(Config), i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp]
    L.simaps_sp_distance.restype = i32
    if hasattr(L, 'simaps_sp_lookup'):  # (ABI 7; absent only in an older revision's A/B build)
        L.simaps_rec_cache_bytes.argtypes = [ctypes.POINTER(Config)]
        L.simaps_rec_cache_bytes.restype = i32
        L.simaps_sp_lookup.argtypes = [ctypes.POINTER(Config), i32, vp, vp, vp, i32, vp, vp]
        L.simaps_sp_lookup.restype = i32
    L.simaps_shortest_path.argtypes = [ctypes.POINTER(Config), i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp]
    L.simaps_shortest_path.restype = i32
    L.simaps_ingest.argtypes = [ctypes.POINTER(Config), ctypes.POINTER(Camera), i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp]
    L.simaps_ingest.restype = i32
    L.simaps_path_mode.argtypes = [i32]
    L.simaps_path_mode.restype = i32
    L.simaps_ingest_chunks.argtypes = [i32, i32]
    L.simaps_ingest_chunks.restype = i32
    L.simaps_sssp_grid.argtypes = [i32, i32, i32, vp, vp, vp, i32, i32, i32, i32, vp]
    L.simaps_sssp_grid.restype = i32
    L.simaps_grid_path.argtypes = [i32, i32, i32, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp]
    L.simaps_grid_path.restype = i32
    L.simaps_fault_status.argtypes = [i32]
    L.simaps_fault_status.restype = i32
    if hasattr(L, 'simaps_build_cspace'):  # (round 6; absent only in an older revision's A/B build)
        L.simaps_occupancy_scatter.argtypes = [ctypes.POINTER(Config), i32, vp, vp, vp, i32, ctypes.c_double, vp, vp]
        L.simaps_occupancy_scatter.restype = i32
        L.simaps_build_cspace.argtypes = [ctypes.POINTER(Config), i32, vp, vp, vp, vp, vp, vp, vp]
        L.simaps_build_cspace.restype = i32
        L.simaps_snap_sources.argtypes = [ctypes.POINTER(Config), i32, vp, vp, vp, vp, vp, i32, vp, vp]
        L.simaps_snap_sources.restype = i32
        L.simaps_global_maps.argtypes = [ctypes.POINTER(Config), i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.simaps_global_maps.restype = i32
    if hasattr(L, 'simaps_ctx_create'):  # (include/simaps_ctx.h; absent only in an older revision's A/B build)
        L.simaps_ctx_create.argtypes = [i32, ctypes.POINTER(vp)]
        L.simaps_ctx_destroy.argtypes = [vp]
        L.simaps_ctx_device.argtypes = [vp]
        L.simaps_ctx_fault_status.argtypes = [vp, i32]
        L.simaps_ctx_fault_info.argtypes = [vp, i32, ctypes.POINTER(i32), ctypes.POINTER(i32)]
        L.simaps_ctx_path_mode.argtypes = [vp, i32]
        for name in CTX_MANAGEMENT:
            getattr(L, name).restype = i32
        for name in CTX_TWINS:  # the context first, then the old entry point's argument list
            twin = getattr(L, 'simaps_ctx_' + name)
            twin.argtypes = [vp] + list(getattr(L, 'simaps_' + name).argtypes)
            twin.restype = i32
    if hasattr(L, 'simaps_store_new_action'):  # (include/simaps_action.h; absent only in an older revision's A/B build)
        L.simaps_action_abi_version.restype = i32
        L.simaps_num_output_channels.argtypes = [i32]
        L.simaps_num_output_channels.restype = i32
        L.simaps_store_new_action.argtypes = [ctypes.POINTER(Config), i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32,
                                              vp, vp, vp, vp, vp, vp, vp]
        L.simaps_store_new_action.restype = i32
        L.simaps_ctx_store_new_action.argtypes = [vp] + list(L.simaps_store_new_action.argtypes)
        L.simaps_ctx_store_new_action.restype = i32
        va = L.simaps_action_abi_version()
        if va != ACTION_ABI_VERSION:
            raise ImportError('libsimaps action ABI version mismatch: %s has %d, this binding is %d'
                              % (path, va, ACTION_ABI_VERSION))
    if hasattr(L, 'simaps_get_state_as'):  # (include/simaps_state16.h; absent only in an older revision's A/B build)
        L.simaps_state16_abi_version.restype = i32
        L.simaps_get_state_as.argtypes = [ctypes.POINTER(Config), i32, vp, vp, vp, vp, vp, vp, vp, i32, i32,
                                          ctypes.POINTER(Debug), vp]
        L.simaps_get_state_as.restype = i32
        L.simaps_ctx_get_state_as.argtypes = [vp] + list(L.simaps_get_state_as.argtypes)
        L.simaps_ctx_get_state_as.restype = i32
        vs = L.simaps_state16_abi_version()
        if vs != STATE16_ABI_VERSION:
            raise ImportError('libsimaps state16 ABI version mismatch: %s has %d, this binding is %d'
                              % (path, vs, STATE16_ABI_VERSION))
    if hasattr(L, 'simaps_get_state_into'):  # (include/simaps_store.h; absent only in an older revision's A/B build)
        L.simaps_store_abi_version.restype = i32
        # simaps_get_state_as's list with capacity and dest after state_dtype
        L.simaps_get_state_into.argtypes = [ctypes.POINTER(Config), i32, vp, vp, vp, vp, vp, vp, vp, i32,
                                            ctypes.c_int64, vp, i32, ctypes.POINTER(Debug), vp]
        L.simaps_get_state_into.restype = i32
        L.simaps_ctx_get_state_into.argtypes = [vp] + list(L.simaps_get_state_into.argtypes)
        L.simaps_ctx_get_state_into.restype = i32
        # simaps_get_state_mixed's list with state_dtype before stream
        L.simaps_get_state_mixed_as.argtypes = list(L.simaps_get_state_mixed.argtypes[:-1]) + [i32, vp]
        L.simaps_get_state_mixed_as.restype = i32
        L.simaps_ctx_get_state_mixed_as.argtypes = [vp] + list(L.simaps_get_state_mixed_as.argtypes)
        L.simaps_ctx_get_state_mixed_as.restype = i32
        vt = L.simaps_store_abi_version()
        if vt != STORE_ABI_VERSION:
            raise ImportError('libsimaps store ABI version mismatch: %s has %d, this binding is %d'
                              % (path, vt, STORE_ABI_VERSION))
    if hasattr(L, 'simaps_get_state_instance'):  # (include/simaps_spec.h; absent only in an older revision's A/B build)
        L.simaps_spec_abi_version.restype = i32
        L.simaps_get_state_instance.argtypes = [ctypes.POINTER(Config), i32]
        L.simaps_get_state_instance.restype = i32
        vk = L.simaps_spec_abi_version()
        if vk != SPEC_ABI_VERSION:
            raise ImportError('libsimaps spec ABI version mismatch: %s has %d, this binding is %d'
                              % (path, vk, SPEC_ABI_VERSION))
    if hasattr(L, 'simaps_get_state_room_class'):  # (include/simaps_spec_room.h; absent only in an older revision's A/B build)
        L.simaps_spec_room_abi_version.restype = i32
        L.simaps_get_state_room_class.argtypes = [ctypes.POINTER(Config), i32]
        L.simaps_get_state_room_class.restype = i32
        vr = L.simaps_spec_room_abi_version()
        if vr != SPEC_ROOM_ABI_VERSION:
            raise ImportError('libsimaps spec_room ABI version mismatch: %s has %d, this binding is %d'
                              % (path, vr, SPEC_ROOM_ABI_VERSION))
    if hasattr(L, 'simaps_get_state_instance_as'):  # (include/simaps_spec_store.h; absent only in an older revision's A/B build)
        L.simaps_spec_store_abi_version.restype = i32
        for f in (L.simaps_get_state_instance_as, L.simaps_get_state_room_class_as):
            f.argtypes = [ctypes.POINTER(Config), i32, i32, i32]
            f.restype = i32
        vs = L.simaps_spec_store_abi_version()
        if vs != SPEC_STORE_ABI_VERSION:
            raise ImportError('libsimaps spec_store ABI version mismatch: %s has %d, this binding is %d'
                              % (path, vs, SPEC_STORE_ABI_VERSION))
    if hasattr(L, 'simaps_get_state_cached'):  # (include/simaps_state_cache.h; absent only in an older revision's A/B build)
        L.simaps_state_cache_abi_version.restype = i32
        L.simaps_state_cache_bytes.argtypes = [ctypes.POINTER(Config)]
        L.simaps_state_cache_bytes.restype = i32
        # simaps_get_state's list with the cache and its record count after stream
        L.simaps_get_state_cached.argtypes = list(L.simaps_get_state.argtypes) + [vp, i32]
        L.simaps_get_state_cached.restype = i32
        L.simaps_ctx_get_state_cached.argtypes = [vp] + list(L.simaps_get_state_cached.argtypes)
        L.simaps_ctx_get_state_cached.restype = i32
        vc = L.simaps_state_cache_abi_version()
        if vc != STATE_CACHE_ABI_VERSION:
            raise ImportError('libsimaps state_cache ABI version mismatch: %s has %d, this binding is %d'
                              % (path, vc, STATE_CACHE_ABI_VERSION))
    if hasattr(L, 'simaps_get_state_into_cached'):  # (include/simaps_state_cache_store.h; absent only in an older revision's A/B build)
        L.simaps_state_cache_store_abi_version.restype = i32
        L.simaps_state_cache_applies.argtypes = [ctypes.POINTER(Config), i32, i32, i32]
        L.simaps_state_cache_applies.restype = i32
        # simaps_get_state_into's / simaps_get_state_as's list with the cache and its record count after stream
        L.simaps_get_state_into_cached.argtypes = list(L.simaps_get_state_into.argtypes) + [vp, i32]
        L.simaps_get_state_as_cached.argtypes = list(L.simaps_get_state_as.argtypes) + [vp, i32]
        for name in ('get_state_into_cached', 'get_state_as_cached'):
            getattr(L, 'simaps_' + name).restype = i32
            twin = getattr(L, 'simaps_ctx_' + name)
            twin.argtypes = [vp] + list(getattr(L, 'simaps_' + name).argtypes)
            twin.restype = i32
        vcs = L.simaps_state_cache_store_abi_version()
        if vcs != STATE_CACHE_STORE_ABI_VERSION:
            raise ImportError('libsimaps state_cache_store ABI version mismatch: %s has %d, this binding is %d'
                              % (path, vcs, STATE_CACHE_STORE_ABI_VERSION))
    if hasattr(L, 'simaps_ingest_seq'):  # (include/simaps_ingest_seq.h; absent only in an older revision's A/B build)
        L.simaps_ingest_seq_abi_version.restype = i32
        # simaps_ingest's list with seq and num_seq after seg_raw
        ing = list(L.simaps_ingest.argtypes)
        L.simaps_ingest_seq.argtypes = ing[:8] + [vp, i32] + ing[8:]
        L.simaps_ingest_seq.restype = i32
        L.simaps_ctx_ingest_seq.argtypes = [vp] + list(L.simaps_ingest_seq.argtypes)
        L.simaps_ctx_ingest_seq.restype = i32
        vq = L.simaps_ingest_seq_abi_version()
        if vq != INGEST_SEQ_ABI_VERSION:
            raise ImportError('libsimaps ingest_seq ABI version mismatch: %s has %d, this binding is %d'
                              % (path, vq, INGEST_SEQ_ABI_VERSION))
    if hasattr(L, 'simaps_store_new_action_as'):  # (include/simaps_action_as.h; absent only in an older revision's A/B build)
        L.simaps_action_as_abi_version.restype = i32
        # simaps_store_new_action's list with q_dtype after q, eps and rng after actions_in, out_explored before stream
        act = list(L.simaps_store_new_action.argtypes)
        L.simaps_store_new_action_as.argtypes = act[:8] + [i32] + act[8:10] + [vp, vp] + act[10:18] + [vp, vp]
        L.simaps_store_new_action_as.restype = i32
        L.simaps_ctx_store_new_action_as.argtypes = [vp] + list(L.simaps_store_new_action_as.argtypes)
        L.simaps_ctx_store_new_action_as.restype = i32
        vx = L.simaps_action_as_abi_version()
        if vx != ACTION_AS_ABI_VERSION:
            raise ImportError('libsimaps action_as ABI version mismatch: %s has %d, this binding is %d'
                              % (path, vx, ACTION_AS_ABI_VERSION))
    v = L.simaps_abi_version()
    if v != ABI_VERSION:
        if os.environ.get('SIMAPS_AB_OLD_ABI') != str(v):
            raise ImportError('libsimaps ABI version mismatch: %s has %d, this binding is %d' % (path, v, ABI_VERSION))
        # SIMAPS_AB_OLD_ABI=<n>: tools/ab_bench.sh timing an older revision's get_state, whose
        # signature is unchanged.  Only the entry points a bench render needs stay callable; any other
        # raises instead of being called with this revision's argument list.
        return _OldAbi(L, v)
    return L


class _OldAbi:
    """An older revision's library bound for an A/B timing only (see _load)."""
    ALLOWED = ('simaps_abi_version', 'simaps_last_error', 'simaps_fault_status', 'simaps_num_channels',
               'simaps_get_state')

    def __init__(self, L, version):
        self._L, self._v = L, version

    def __getattr__(self, name):
        if name in self.ALLOWED:
            return getattr(self._L, name)
        raise SimapsError('%s is not callable on the ABI-%d library loaded for an A/B timing (SIMAPS_AB_OLD_ABI); '
                          'only %s are' % (name, self._v, ', '.join(self.ALLOWED)))


lib = _load()


def has_entry(name, L=None):
    """Whether the library exports simaps_<name> (an older revision's A/B build may lack a newer header's)."""
    try:
        return hasattr(L or lib, 'simaps_' + name)
    except SimapsError:
        return False

EXPORTED = ('simaps_abi_version', 'simaps_last_error', 'simaps_fault_status', 'simaps_num_channels',
            'simaps_robot_mask', 'simaps_pack_robots', 'simaps_get_state', 'simaps_sp_distance', 'simaps_shortest_path', 'simaps_ingest', 'simaps_ingest_chunks', 'simaps_path_mode',
            'simaps_sssp_grid', 'simaps_grid_path', 'simaps_rec_cache_bytes', 'simaps_sp_lookup',
            'simaps_get_state_mixed', 'simaps_source_hash', 'simaps_occupancy_scatter', 'simaps_build_cspace',
            'simaps_snap_sources', 'simaps_global_maps')

# error codes and device fault bits (include/simaps.h)
EINVAL, EUNSUPPORTED, EHIP, EDEVICE = -1, -2, -3, -4
FAULT_TIMEOUT, FAULT_ROUNDS, FAULT_DESCRIPTOR = 1, 2, 4


class DeviceFault(SimapsError):
    """A kernel reported SIMAPS_FAULT_* bits: the outputs of that launch are invalid."""


def check(rc, L=None):
    if rc != 0:
        L = L or lib
        cls = DeviceFault if rc == EDEVICE else SimapsError
        raise cls('libsimaps error %d: %s' % (rc, L.simaps_last_error().decode()))


def check_faults(L=None):
    """Raise DeviceFault if a completed launch reported a device-side fault (clears the word).
    Call after the stream has been synchronised (e.g. after a device->host copy of the results)."""
    L = L or lib
    f = L.simaps_fault_status(1)
    if f < 0:
        check(f, L)
    if f:
        raise DeviceFault('device fault bits 0x%x (%s): the outputs of a completed launch are invalid' % (
            f, ' '.join(n for b, n in ((FAULT_TIMEOUT, 'barrier-timeout'), (FAULT_ROUNDS, 'sssp-round-cap'),
                                       (FAULT_DESCRIPTOR, 'descriptor-clamped')) if f & b)))


def call(context, name, *args, L=None):
    """The entry point simaps_<name> on the default context (context None), or its twin
    simaps_ctx_<name> through `context` (a simaps.context.Context); returns the return code."""
    L = L or lib
    if context is None:
        return getattr(L, 'simaps_' + name)(*args)
    return getattr(L, 'simaps_ctx_' + name)(context.handle, *args)


def check_context_faults(context=None, L=None):
    """check_faults() for the default context, context.check_faults() for a created one."""
    if context is None:
        check_faults(L)
    else:
        context.check_faults()


def stream_handle(stream=None):
    s = stream if stream is not None else torch.cuda.current_stream()
    return ctypes.c_void_p(s.cuda_stream)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def robot_mask(robot_type, with_cube=False):
    out = np.zeros((96, 96), dtype=np.float32)
    check(lib.simaps_robot_mask(TYPE_IDS.get(robot_type, robot_type), int(with_cube), out.ctypes.data))
    return out
