"""CPU: the state cache's C ABI for the store launches and the 16-bit launches
(include/simaps_state_cache_store.h) -- declared, exported, bound, part of the build and of the source
hash; the argument checks that need no GPU; which calls use a cache they are given
(simaps_state_cache_applies) against tests/state_cache_model.py.  The older headers are untouched
(simaps_abi_version stays 8, simaps_state_cache_abi_version 1).

No kernel is launched here."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import state_cache_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'simaps_state_cache_store.h')
WANT = sorted(['simaps_state_cache_store_abi_version', 'simaps_state_cache_applies', 'simaps_get_state_into_cached',
               'simaps_ctx_get_state_into_cached', 'simaps_get_state_as_cached', 'simaps_ctx_get_state_as_cached'])
UNITS = ['simaps_spec_cached_store_f32.hip', 'simaps_spec_cached_store_bf16.hip', 'simaps_spec_cached_store_f16.hip']
F32, BF16, F16 = 0, 1, 2
FLAGSHIP = 'lifting_4-small_divider'
# the room origins of tests/test_gpu_room_origin.py
ORIGINS = [(70, 68), (70, 69), (70, 71), (70, 72), (68, 70), (72, 70), (70, 98), (70, 99), (70, 7), (70, 6),
           (0, 0), (140, 140), (3, 70), (137, 70)]


@pytest.fixture(scope='module')
def L():
    from simaps import _lib
    return _lib


def _cfg(name, layout='chw'):
    from simaps import batch, constants as K, synthetic
    length, width, _ = K.room_dims(synthetic.CONFIGS[name]['env_name'])
    return batch.make_config(synthetic.config_flags(name), width, length, layout, 'fma')


def _text(path=HEADER):
    return re.sub(r'/\*.*?\*/', '', open(path).read(), flags=re.S)


def test_header_library_and_binding_agree(L):
    txt = _text()
    assert sorted(set(re.findall(r'\b(simaps_[a-z_0-9]+)\s*\(', txt))) == WANT == sorted(L.EXPORTED_STATE_CACHE_STORE)
    assert int(re.search(r'#define SIMAPS_STATE_CACHE_STORE_ABI_VERSION (\d+)', txt).group(1)) == 1
    assert L.STATE_CACHE_STORE_ABI_VERSION == 1 and L.lib.simaps_state_cache_store_abi_version() == 1
    for name in WANT:                                                    # exported by the library, and bound
        assert isinstance(getattr(L.lib, name), ctypes._CFuncPtr), name
        assert getattr(L.lib, name).restype is ctypes.c_int, name
    for other in (L.EXPORTED, L.EXPORTED_CTX, L.EXPORTED_ACTION, L.EXPORTED_STATE16, L.EXPORTED_STORE, L.EXPORTED_SPEC,
                  L.EXPORTED_SPEC_ROOM, L.EXPORTED_SPEC_STORE, L.EXPORTED_STATE_CACHE, L.EXPORTED_INGEST_SEQ,
                  L.EXPORTED_ACTION_AS):
        assert not set(L.EXPORTED_STATE_CACHE_STORE) & set(other)
    # the older headers are untouched
    assert L.lib.simaps_abi_version() == 8 and L.lib.simaps_state_cache_abi_version() == 1
    assert L.lib.simaps_store_abi_version() == 1 and L.lib.simaps_state16_abi_version() == 1
    assert L.lib.simaps_spec_store_abi_version() == 1 and L.lib.simaps_spec_abi_version() == 1
    assert L.lib.simaps_spec_room_abi_version() == 1
    assert L.has_entry('get_state_into_cached') and L.has_entry('get_state_as_cached')
    assert L.has_entry('ctx_get_state_into_cached') and L.has_entry('ctx_get_state_as_cached')


def test_cached_entries_take_the_uncached_arguments_plus_the_cache(L):
    for name, hdr in (('get_state_into', 'simaps_store.h'), ('get_state_as', 'simaps_state16.h')):
        base = list(getattr(L.lib, 'simaps_' + name).argtypes)
        assert list(getattr(L.lib, 'simaps_%s_cached' % name).argtypes) == base + [ctypes.c_void_p, ctypes.c_int32]
        assert list(getattr(L.lib, 'simaps_ctx_%s_cached' % name).argtypes) == \
            [ctypes.c_void_p] + base + [ctypes.c_void_p, ctypes.c_int32]
        names = lambda s: [a.split()[-1].lstrip('*') for a in s.replace('\n', ' ').split(',')]  # noqa: E731
        decl = re.search(r'int simaps_%s_cached\((.*?)\);' % name, _text(), re.S).group(1)
        plain = re.search(r'int simaps_%s\((.*?)\);' % name, _text(os.path.join(ROOT, 'include', hdr)), re.S).group(1)
        assert names(decl) == names(plain) + ['cache', 'cache_records'], name
        ctx = re.search(r'int simaps_ctx_%s_cached\((.*?)\);' % name, _text(), re.S).group(1)
        assert names(ctx) == ['ctx'] + names(decl), name


def test_header_and_units_are_part_of_the_build_and_the_source_hash():
    from simaps import _srchash
    rels = [rel for rel, _ in _srchash.source_files()]
    assert 'include/simaps_state_cache_store.h' in rels
    for f in UNITS + ['simaps_spec_cached_store.inc', 'state_cache_store.h']:
        assert 'csrc/' + f in rels, f
    mk = open(os.path.join(ROOT, 'spatial-intention-maps_amd', 'csrc', 'Makefile')).read()
    srcs = re.search(r'^SRCS\s*:=(.*)$', mk, re.M).group(1)
    deps = re.search(r'^DEPS\s*:=(.*)$', mk, re.M).group(1)
    for u in UNITS:
        assert u in srcs, u                                              # so `make diag` and `make prof` build them too
    for d in ('include/simaps_state_cache_store.h', 'simaps_spec_cached_store.inc', 'state_cache_store.h'):
        assert d in deps, d
    assert re.search(r'^resources_spec_cached_store:', mk, re.M)
    for u in UNITS:                                                      # one element type per unit, one shared body
        src = open(os.path.join(ROOT, 'spatial-intention-maps_amd', 'csrc', u)).read()
        assert re.search(r'^#define SIMAPS_STORE_DTYPE [012]$', src, re.M) and 'simaps_spec_cached_store.inc' in src


def test_argument_checks_launch_nothing(L):
    c = _cfg(FLAGSHIP)
    into, plain = L.lib.simaps_get_state_into_cached, L.lib.simaps_get_state_as_cached
    ia = (c, 0, None, None, None, None, None, None, None)                # cfg, N = 0, the seven buffers, the store
    for dt in (F32, BF16, F16):
        assert into(*ia, dt, 0, None, 0, None, None, 8, 1) == L.EINVAL                           # misaligned cache
        assert b'aligned' in L.lib.simaps_last_error()
        assert into(*ia, dt, 0, None, 0, None, None, None, -1) == L.EINVAL                       # cache_records < 0
        assert b'cache_records' in L.lib.simaps_last_error()
        assert into(*ia, dt, 0, None, 0, None, None, None, 0) == 0                               # N == 0: nothing to do
        assert into(*ia, dt, 0, None, 0, None, None, 16, 4) == 0                                 # aligned, never used
        assert plain(*ia, dt, 0, None, None, 8, 1) == L.EINVAL
        assert plain(*ia, dt, 0, None, None, None, -1) == L.EINVAL
        assert plain(*ia, dt, 0, None, None, None, 0) == 0
    for dt in (-1, 3, 7):
        assert into(*ia, dt, 0, None, 0, None, None, None, 0) == L.EINVAL                        # a bad dtype
        assert b'state_dtype' in L.lib.simaps_last_error()
        assert plain(*ia, dt, 0, None, None, None, 0) == L.EINVAL
    # N > 0 with a bad cache: refused before a NULL buffer could be looked at
    assert into(c, 4, None, None, None, None, None, None, None, BF16, 0, None, 0, None, None, 8, 4) == L.EINVAL
    assert b'aligned' in L.lib.simaps_last_error()
    assert plain(c, 4, None, None, None, None, None, None, None, BF16, 0, None, None, None, -2) == L.EINVAL
    assert into(None, 0, None, None, None, None, None, None, None, F32, 0, None, 0, None, None, None, 0) == L.EINVAL
    # the context twins check the same before they resolve the context
    assert L.lib.simaps_ctx_get_state_into_cached(None, *ia, BF16, 0, None, 0, None, None, 8, 1) == L.EINVAL
    assert L.lib.simaps_ctx_get_state_as_cached(None, *ia, F16, 0, None, None, None, -1) == L.EINVAL


def test_applies_truth_table(L):
    q = L.lib.simaps_state_cache_applies
    c, hwc = _cfg(FLAGSHIP), _cfg(FLAGSHIP, 'hwc')
    kinds = [(F32, 1), (BF16, 0), (F16, 0), (BF16, 1), (F16, 1)]
    for dt, into in kinds + [(F32, 0)]:
        assert q(c, dt, into, 0) == 1, (dt, into)
        assert q(c, dt, 2 * into, 0) == q(c, dt, -into, 0) == 1                                   # into by truthiness
        assert q(hwc, dt, into, 0) == 0, (dt, into)
        for dbg in (1, 2, -1):
            assert q(c, dt, into, dbg) == 0, (dt, into, dbg)
        assert q(_cfg('rescue_4-small_empty'), dt, into, 0) == 0                                  # S2: one source
        assert q(_cfg('pushing_4-large_empty'), dt, into, 0) == 0 and q(_cfg('lifting_4-large_doors'), dt, into, 0) == 0
        d = _cfg(FLAGSHIP)
        d.room_j0 = 6                                                    # the window would start left of the map
        assert q(d, dt, into, 0) == 0, (dt, into)
        d.room_j0 = 7
        assert q(d, dt, into, 0) == 1, (dt, into)
        for f in ('H', 'W', 'room_h', 'room_w'):                         # one cell off the room class
            e = _cfg(FLAGSHIP)
            setattr(e, f, getattr(e, f) + 1)
            assert q(e, dt, into, 0) == 0, (dt, into, f)
    assert L.lib.simaps_get_state_instance_as(_cfg('rescue_4-small_empty'), BF16, 1, 0) == L.SPEC_S2
    for i0, j0 in ORIGINS:                                               # every kind follows the float32 rule's origins
        d = _cfg(FLAGSHIP)
        d.room_i0, d.room_j0 = i0, j0
        want = int(M.uses_cache(d))
        assert want == int(j0 >= 7 and ((j0 - 7) & ~3) + 144 <= d.W)
        assert q(d, F32, 0, 0) == want, (i0, j0)
        assert q(d, F32, 0, 1) == int(M.uses_cache(d, debug=True)) == 0
        for dt, into in kinds:
            assert q(d, dt, into, 0) == want, (i0, j0, dt, into)
    for dt in (-1, 3, 1 << 20):
        assert q(c, dt, 0, 0) == q(c, dt, 1, 0) == L.EINVAL
    assert q(None, F32, 0, 0) == q(None, BF16, 1, 1) == L.EINVAL and L.EINVAL < 0


def test_state_batch_follows_the_library(L):
    from simaps import batch
    c = _cfg(FLAGSHIP)

    class B:  # the fields uses_state_cache reads
        cfg, flags, _rec = c, {'use_shortest_path_to_receptacle_map': True}, None
    uses = batch.StateBatch.uses_state_cache
    for dt in (None, torch.float32, torch.bfloat16, torch.float16):
        for into in (False, True):
            assert uses(B, dtype=dt, into=into) is True
            assert uses(B, dtype=dt, into=into, debug=True) is False
            assert uses(B, dtype=dt, into=into, debug={'status': object()}) is False
            assert uses(B, dtype=dt, into=into, debug={'status': None}) is True
    with pytest.raises(ValueError):
        uses(B, dtype=torch.float64)
    B._rec = object()                                                    # an enabled receptacle cache is a debug output of render()
    assert uses(B, dtype=torch.bfloat16) is False and uses(B, dtype=torch.bfloat16, into=True) is True
    B.cfg, B._rec = _cfg(FLAGSHIP, 'hwc'), None
    assert uses(B, dtype=torch.float16, into=True) is False
    # which launches pass the cache: the call's state_cache= first, else the batch's (True: the float32 render only)
    on = batch.StateBatch._state_cache_on
    for batch_wide, want in ((True, (True, False)), ('all', (True, True)), (False, (False, False))):
        B.state_cache = batch_wide
        assert (on(B, None, True), on(B, None, False)) == want, batch_wide
        assert on(B, True, True) and on(B, True, False) and not on(B, False, True) and not on(B, False, False)
    from simaps import synthetic
    for bad in ('ALL', 'store', '', 'true'):                             # a string other than 'all' is refused, before any device use
        with pytest.raises(ValueError, match='state_cache'):
            batch.StateBatch([synthetic.make_scene(FLAGSHIP, 0)], device='cpu', state_cache=bad)
    sig = inspect.signature(batch.StateBatch.render_into).parameters
    assert sig['state_cache'].default is None and list(sig)[-1] == 'state_cache'
    assert inspect.signature(batch.StateBatch.uses_state_cache).parameters['dtype'].default is None
