"""CPU: the context-scoped C ABI (include/simaps_ctx.h) is declared, exported and bound; handles are
validated; argument checks come before any device use.

No kernel is launched here (no GPU in the CPU tier): a host without a GPU gets SIMAPS_EHIP from
simaps_ctx_create, never a crash."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'simaps_ctx.h')

MANAGEMENT = ['simaps_ctx_create', 'simaps_ctx_destroy', 'simaps_ctx_device', 'simaps_ctx_fault_status',
              'simaps_ctx_fault_info', 'simaps_ctx_path_mode']
TWINS = ['get_state', 'get_state_mixed', 'sp_distance', 'sp_lookup', 'shortest_path', 'ingest', 'sssp_grid',
         'grid_path', 'occupancy_scatter', 'build_cspace', 'snap_sources', 'global_maps']
WANT = sorted(MANAGEMENT + ['simaps_ctx_' + n for n in TWINS])


def declared_symbols():
    """Every simaps_* name followed by `(` anywhere in the header, comments included (the rule of
    tests/test_abi.py)."""
    txt = open(HEADER).read()
    return sorted(set(re.findall(r'\b(simaps_[a-z_0-9]+)\s*\(', txt)))


@pytest.fixture(scope='module')
def L():
    from simaps import _lib
    return _lib


def test_header_declares_the_context_abi():
    assert declared_symbols() == WANT
    assert '#include "simaps.h"' in open(HEADER).read()


def test_library_exports_every_declared_symbol(L):
    for name in declared_symbols():
        assert hasattr(L.lib, name), name
        assert isinstance(getattr(L.lib, name), ctypes._CFuncPtr)
    assert sorted(L.EXPORTED_CTX) == WANT
    assert not set(L.EXPORTED_CTX) & set(L.EXPORTED)
    # each twin takes the context, then the old entry point's argument list
    for n in TWINS:
        assert getattr(L.lib, 'simaps_ctx_' + n).argtypes[1:] == getattr(L.lib, 'simaps_' + n).argtypes


def test_kernel_id_table_matches_header(L):
    txt = open(HEADER).read()
    ids = {int(v): k.lower() for k, v in re.findall(r'#define SIMAPS_K_([A-Z_]+) (\d+)', txt) if k != 'COUNT'}
    assert ids == L.K_NAMES
    assert sorted(ids) == list(range(1, len(ids) + 1))          # ids start at 1: a posted word is never 0
    assert int(re.search(r'#define SIMAPS_K_COUNT (\d+)', txt).group(1)) == len(ids)


def test_header_is_part_of_the_source_hash():
    from simaps import _srchash
    assert 'include/simaps_ctx.h' in [rel for rel, _ in _srchash.source_files()]


def test_bad_handles_are_refused_not_followed(L):
    lib = L.lib
    buf = ctypes.create_string_buffer(4096)                      # live memory that is not a context
    fake = ctypes.c_void_p(ctypes.addressof(buf))
    assert lib.simaps_ctx_fault_status(fake, 0) == L.EINVAL
    assert b'not a live context' in lib.simaps_last_error()
    assert lib.simaps_ctx_path_mode(fake, 1) == L.EINVAL
    assert lib.simaps_ctx_device(fake) == L.EINVAL
    assert lib.simaps_ctx_destroy(fake) == L.EINVAL
    k, u = ctypes.c_int(7), ctypes.c_int(7)
    assert lib.simaps_ctx_fault_info(fake, 1, ctypes.byref(k), ctypes.byref(u)) == L.EINVAL
    assert (k.value, u.value) == (-1, -1)
    cfg = L.Config()
    assert lib.simaps_ctx_get_state(fake, cfg, 1, None, None, None, None, None, None, None, 0, None, None) == L.EINVAL
    assert b'not a live context' in lib.simaps_last_error()
    assert buf.raw == b'\0' * 4096                               # nothing was written through the pointer
    assert lib.simaps_ctx_destroy(None) == L.EINVAL


def test_create_argument_checks(L):
    lib = L.lib
    h = ctypes.c_void_p(0xdead)
    assert lib.simaps_ctx_create(-7, ctypes.byref(h)) == L.EINVAL
    assert not h.value
    assert lib.simaps_ctx_create(0, None) == L.EINVAL
    h = ctypes.c_void_p(0xdead)
    rc = lib.simaps_ctx_create(0, ctypes.byref(h))
    if rc == 0:
        assert h.value
        assert lib.simaps_ctx_device(h) == 0
        assert lib.simaps_ctx_path_mode(h, 2) == 0 and lib.simaps_ctx_path_mode(h, 0) == 2
        assert lib.simaps_ctx_path_mode(h, 4) == L.EINVAL
        assert lib.simaps_ctx_destroy(h) == 0
        assert lib.simaps_ctx_destroy(h) == L.EINVAL             # a second destroy of the same handle
        assert lib.simaps_ctx_device(h) == L.EINVAL
    else:                                                        # the CPU-only host
        assert rc == L.EHIP
        assert not h.value


def test_null_context_is_the_default_context(L):
    lib = L.lib
    prev = lib.simaps_path_mode(0)
    try:
        assert lib.simaps_ctx_path_mode(None, 1) == 0            # the previous process-wide mode
        assert lib.simaps_path_mode(0) == 1                      # one setting under both names
        assert lib.simaps_ctx_path_mode(None, 0) == 0
        assert lib.simaps_ctx_path_mode(None, 9) == L.EINVAL
        assert lib.simaps_ctx_device(None) == -1                 # no device of its own
    finally:
        lib.simaps_path_mode(prev)


def test_argument_checks_come_before_any_device_use(L):
    """The same codes as the old names, on a host with or without a GPU."""
    from simaps import batch, constants as K
    lib = L.lib
    cfg = batch.make_config(dict(K.DEFAULT_FLAGS), 1.0, 0.5)
    assert lib.simaps_get_state(cfg, -1, None, None, None, None, None, None, None, 0, None, None) == L.EINVAL
    assert lib.simaps_ctx_get_state(None, cfg, -1, None, None, None, None, None, None, None, 0, None, None) == L.EINVAL
    assert b'N < 0' in lib.simaps_last_error()
    assert lib.simaps_sp_lookup(None, 1, None, None, None, 1, None, None) == L.EINVAL
    assert lib.simaps_ctx_sp_lookup(None, None, 1, None, None, None, 1, None, None) == L.EINVAL
    assert b'cfg is NULL' in lib.simaps_last_error()


def test_python_context_refuses_the_cpu():
    from simaps import context
    with pytest.raises(ValueError):
        context.Context(device='cpu')
