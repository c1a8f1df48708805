"""CPU: the store C ABI (include/simaps_store.h: simaps_get_state_into, simaps_get_state_mixed_as and
their context twins) is declared, exported and bound; the older headers keep their versions; every
argument check comes before any device use, so none of this needs (or touches) a GPU.

No kernel is launched here."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'simaps_store.h')
WANT = sorted(['simaps_store_abi_version', 'simaps_get_state_into', 'simaps_ctx_get_state_into',
               'simaps_get_state_mixed_as', 'simaps_ctx_get_state_mixed_as'])


@pytest.fixture(scope='module')
def L():
    from simaps import _lib
    return _lib


def declared_symbols(path):
    """Every simaps_* name followed by `(` in the header outside its comments."""
    txt = re.sub(r'/\*.*?\*/', '', open(path).read(), flags=re.S)
    return sorted(set(re.findall(r'\b(simaps_[a-z_0-9]+)\s*\(', txt)))


def test_header_declares_exactly_the_store_abi(L):
    txt = open(HEADER).read()
    assert declared_symbols(HEADER) == WANT
    assert '#include "simaps_state16.h"' in txt
    assert int(re.search(r'#define SIMAPS_STORE_ABI_VERSION (\d+)', txt).group(1)) == L.STORE_ABI_VERSION == 1
    assert L.lib.simaps_store_abi_version() == 1
    assert 'race' in txt                                                # the duplicate-destination contract is stated


def test_older_headers_keep_their_versions_and_symbols(L):
    assert L.lib.simaps_abi_version() == 8
    assert L.lib.simaps_action_abi_version() == 1
    assert L.lib.simaps_state16_abi_version() == 1
    inc = os.path.join(ROOT, 'include')
    assert declared_symbols(os.path.join(inc, 'simaps_state16.h')) == sorted(L.EXPORTED_STATE16)
    assert declared_symbols(os.path.join(inc, 'simaps_ctx.h')) == sorted(L.EXPORTED_CTX)
    assert declared_symbols(os.path.join(inc, 'simaps_action.h')) == sorted(L.EXPORTED_ACTION)
    ctx = open(os.path.join(inc, 'simaps_ctx.h')).read()
    assert re.search(r'#define SIMAPS_K_GET_STATE_INTO 13\b', ctx) and re.search(r'#define SIMAPS_K_COUNT 13\b', ctx)
    assert L.K_NAMES[13] == 'get_state_into' and len(L.K_NAMES) == 13
    assert 'simaps_store.h' in open(os.path.join(inc, 'simaps_state16.h')).read()


def test_library_exports_and_binds_the_store_abi(L):
    for name in WANT:
        assert isinstance(getattr(L.lib, name), ctypes._CFuncPtr), name
    assert sorted(L.EXPORTED_STORE) == WANT
    for other in (L.EXPORTED, L.EXPORTED_CTX, L.EXPORTED_ACTION, L.EXPORTED_STATE16):
        assert not set(L.EXPORTED_STORE) & set(other)
    into, twin = L.lib.simaps_get_state_into.argtypes, L.lib.simaps_ctx_get_state_into.argtypes
    assert len(into) == 15
    assert twin[0] is ctypes.c_void_p and list(twin[1:]) == list(into)
    # simaps_get_state_as's list with capacity (int64) and dest after state_dtype
    as_ = list(L.lib.simaps_get_state_as.argtypes)
    assert list(into) == as_[:10] + [ctypes.c_int64, ctypes.c_void_p] + as_[10:]
    mixed, mtwin = L.lib.simaps_get_state_mixed_as.argtypes, L.lib.simaps_ctx_get_state_mixed_as.argtypes
    old = list(L.lib.simaps_get_state_mixed.argtypes)
    assert list(mixed) == old[:-1] + [ctypes.c_int, old[-1]] and len(mixed) == 16
    assert mtwin[0] is ctypes.c_void_p and list(mtwin[1:]) == list(mixed)
    # reachable through _lib.call on the default context (a context twin takes the handle first)
    assert L.call(None, 'get_state_into', *_into_args(L, N=0)) == 0
    assert L.call(None, 'get_state_mixed_as', *_mixed_args(L, N=0)) == 0


def test_new_sources_are_part_of_the_source_hash():
    from simaps import _srchash
    rels = [rel for rel, _ in _srchash.source_files()]
    for rel in ('include/simaps_store.h', 'csrc/store.h', 'csrc/simaps_store.inc', 'csrc/simaps_store_f32.hip',
                'csrc/simaps_store_bf16.hip', 'csrc/simaps_store_f16.hip'):
        assert rel in rels, rel
    assert len([r for r in rels if r.startswith('csrc/simaps_store_')]) == 3   # one unit per element type
    mk = open(os.path.join(ROOT, 'spatial-intention-maps_amd', 'csrc', 'Makefile')).read()
    srcs = re.search(r'^SRCS\s*:=(.*)$', mk, re.M).group(1)
    deps = re.search(r'^DEPS\s*:=(.*)$', mk, re.M).group(1)
    for unit in ('simaps_store_f32.hip', 'simaps_store_bf16.hip', 'simaps_store_f16.hip'):
        assert unit in srcs
    assert 'simaps_store.inc' in deps and 'store.h' in deps and 'include/simaps_store.h' in deps
    assert re.search(r'^resources_store:', mk, re.M)


D = ctypes.c_void_p(0x1000)   # a plausible non-NULL dummy: never dereferenced, every call here fails its checks first


def _into_args(L, **kw):
    from simaps import batch, constants as K
    a = dict(cfg=batch.make_config(dict(K.DEFAULT_FLAGS), 1.0, 0.5), N=1, agents=D, envs=D, robots=D, paths=D,
             occupancy=D, overhead=D, store=D, state_dtype=L.STATE_BF16, capacity=4, dest=D, num_robots_per_env=0,
             dbg=None, stream=None)
    a.update(kw)
    return [a[k] for k in ('cfg', 'N', 'agents', 'envs', 'robots', 'paths', 'occupancy', 'overhead', 'store',
                           'state_dtype', 'capacity', 'dest', 'num_robots_per_env', 'dbg', 'stream')]


def _into(L, ctx=None, twin=False, **kw):
    if twin:
        return L.lib.simaps_ctx_get_state_into(ctx, *_into_args(L, **kw))
    return L.lib.simaps_get_state_into(*_into_args(L, **kw))


_KEEP = []


def _mixed_args(L, **kw):
    from simaps import batch, constants as K
    cfgs = (L.Config * 2)(batch.make_config(dict(K.DEFAULT_FLAGS), 1.0, 0.5),
                          batch.make_config(dict(K.DEFAULT_FLAGS), 1.0, 1.0))
    nrs = np.zeros(2, np.int32)
    _KEEP.append((cfgs, nrs))
    a = dict(cfgs=cfgs, nrs=nrs.ctypes.data, n_cfgs=2, N=1, agents=D, agent_cfg=D, envs=D, robots=D, paths=D,
             occupancy=D, map_off=D, overhead=D, state=D, out_off=D, state_dtype=L.STATE_F16, stream=None)
    a.update(kw)
    return [a[k] for k in ('cfgs', 'nrs', 'n_cfgs', 'N', 'agents', 'agent_cfg', 'envs', 'robots', 'paths', 'occupancy',
                           'map_off', 'overhead', 'state', 'out_off', 'state_dtype', 'stream')]


def _mixed(L, ctx=None, twin=False, **kw):
    if twin:
        return L.lib.simaps_ctx_get_state_mixed_as(ctx, *_mixed_args(L, **kw))
    return L.lib.simaps_get_state_mixed_as(*_mixed_args(L, **kw))


@pytest.mark.parametrize('twin', [False, True], ids=['plain', 'ctx'])
def test_get_state_into_argument_errors_come_before_any_device_use(L, twin):
    from simaps import batch, constants as K
    err = L.lib.simaps_last_error
    for bad in (-1, 3, 99):
        assert _into(L, twin=twin, state_dtype=bad) == L.EINVAL, bad
        assert b'unknown state_dtype %d' % bad in err()
    assert _into(L, twin=twin, state_dtype=7, N=0) == L.EINVAL            # an unknown dtype even with nothing to do
    for dt in (L.STATE_F32, L.STATE_BF16, L.STATE_F16):
        assert _into(L, twin=twin, state_dtype=dt, store=None) == L.EINVAL
        assert b'store is NULL' in err()
        for off in (2, 4, 8, 12):
            assert _into(L, twin=twin, state_dtype=dt, store=ctypes.c_void_p(0x1000 + off)) == L.EINVAL, off
            assert b'not aligned to 16 bytes' in err()
        for cap in (-1, -2 ** 40):
            assert _into(L, twin=twin, state_dtype=dt, capacity=cap) == L.EINVAL
            assert b'capacity' in err() and b'< 0' in err()
        assert _into(L, twin=twin, state_dtype=dt, capacity=-1, N=0) == L.EINVAL
        assert _into(L, twin=twin, state_dtype=dt, dest=None) == L.EINVAL
        assert b'dest is NULL' in err()
        assert _into(L, twin=twin, state_dtype=dt, dest=None, capacity=0, store=None) == L.EINVAL
        assert b'dest is NULL' in err()
        # everything simaps_get_state refuses
        assert _into(L, twin=twin, state_dtype=dt, cfg=None) == L.EINVAL
        assert b'cfg is NULL' in err()
        assert _into(L, twin=twin, state_dtype=dt, N=-1) == L.EINVAL
        assert b'N < 0' in err()
        for name in ('agents', 'envs', 'robots', 'occupancy', 'overhead'):
            assert _into(L, twin=twin, state_dtype=dt, **{name: None}) == L.EINVAL, name
            assert b'NULL buffer' in err()
        flags = dict(K.DEFAULT_FLAGS, use_intention_map=True)
        assert _into(L, twin=twin, state_dtype=dt, cfg=batch.make_config(flags, 1.0, 0.5), paths=None) == L.EINVAL
        assert b'paths is NULL' in err()
        flags = dict(K.DEFAULT_FLAGS, use_intention_channels=True)
        for nr in (0, 9):
            assert _into(L, twin=twin, state_dtype=dt, cfg=batch.make_config(flags, 1.0, 0.5),
                         num_robots_per_env=nr) == L.EINVAL
            assert b'intention channels need num_robots_per_env' in err()
        bad_cfg = batch.make_config(dict(K.DEFAULT_FLAGS), 1.0, 0.5)
        bad_cfg.H = 0
        assert _into(L, twin=twin, state_dtype=dt, cfg=bad_cfg) == L.EINVAL
        assert b'bad grid' in err()
        # N == 0: nothing to do, nothing touched
        assert _into(L, twin=twin, state_dtype=dt, N=0) == 0
        assert _into(L, twin=twin, state_dtype=dt, N=0, store=None, dest=None, capacity=0) == 0
        assert _into(L, twin=twin, state_dtype=dt, N=0, store=ctypes.c_void_p(0x1004), dest=None) == 0


@pytest.mark.parametrize('twin', [False, True], ids=['plain', 'ctx'])
def test_get_state_mixed_as_argument_errors_come_before_any_device_use(L, twin):
    err = L.lib.simaps_last_error
    for bad in (-1, 3, 99):
        assert _mixed(L, twin=twin, state_dtype=bad) == L.EINVAL, bad
        assert b'unknown state_dtype %d' % bad in err()
    assert _mixed(L, twin=twin, state_dtype=7, N=0) == L.EINVAL
    for dt in (L.STATE_F32, L.STATE_BF16, L.STATE_F16):
        assert _mixed(L, twin=twin, state_dtype=dt, state=None) == L.EINVAL
        assert b'state is NULL' in err()
        for off in (2, 4, 8, 12):
            assert _mixed(L, twin=twin, state_dtype=dt, state=ctypes.c_void_p(0x1000 + off)) == L.EINVAL, off
            assert b'not aligned to 16 bytes' in err()
        # everything simaps_get_state_mixed refuses
        assert _mixed(L, twin=twin, state_dtype=dt, cfgs=None) == L.EINVAL
        for n in (0, L.MAX_MIXED + 1):
            assert _mixed(L, twin=twin, state_dtype=dt, n_cfgs=n) == L.EINVAL
            assert b'n_cfgs' in err()
        assert _mixed(L, twin=twin, state_dtype=dt, N=-1) == L.EINVAL
        assert b'N < 0' in err()
        for name in ('agents', 'agent_cfg', 'envs', 'robots', 'occupancy', 'map_off', 'overhead', 'out_off'):
            assert _mixed(L, twin=twin, state_dtype=dt, **{name: None}) == L.EINVAL, name
            assert b'NULL buffer' in err()
        assert _mixed(L, twin=twin, state_dtype=dt, N=0) == 0
        assert _mixed(L, twin=twin, state_dtype=dt, N=0, state=None) == 0


def test_stale_context_handle_is_refused(L):
    buf = ctypes.create_string_buffer(4096)                             # live memory that is not a context
    fake = ctypes.c_void_p(ctypes.addressof(buf))
    assert _into(L, ctx=fake, twin=True) == L.EINVAL
    assert b'not a live context' in L.lib.simaps_last_error()
    assert _mixed(L, ctx=fake, twin=True) == L.EINVAL
    assert b'not a live context' in L.lib.simaps_last_error()
    assert buf.raw == b'\0' * 4096
