"""CPU: the state cache's C ABI (include/simaps_state_cache.h) -- declared, exported, bound, part of the
source hash; the record header's layout and the record's size; the argument checks that need no GPU.
The older headers are untouched (simaps_abi_version stays 8).

No kernel is launched here."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'simaps_state_cache.h')
WANT = sorted(['simaps_state_cache_abi_version', 'simaps_state_cache_bytes', 'simaps_get_state_cached',
               'simaps_ctx_get_state_cached'])


@pytest.fixture(scope='module')
def L():
    from simaps import _lib
    return _lib


def _cfg(name, layout='chw'):
    from simaps import batch, constants as K, synthetic
    length, width, _ = K.room_dims(synthetic.CONFIGS[name]['env_name'])
    return batch.make_config(synthetic.config_flags(name), width, length, layout, 'fma')


def _header_text():
    return re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)


def test_header_declares_exactly_the_entry_points(L):
    txt = _header_text()
    assert sorted(set(re.findall(r'\b(simaps_[a-z_0-9]+)\s*\(', txt))) == WANT == sorted(L.EXPORTED_STATE_CACHE)
    assert int(re.search(r'#define SIMAPS_STATE_CACHE_ABI_VERSION (\d+)', txt).group(1)) == L.STATE_CACHE_ABI_VERSION
    assert int(re.search(r'#define SIMAPS_STATE_CACHE_MAGIC (0x[0-9a-fA-F]+)', txt).group(1), 16) == L.STATE_CACHE_MAGIC
    assert L.lib.simaps_state_cache_abi_version() == L.STATE_CACHE_ABI_VERSION
    for name in WANT:
        assert isinstance(getattr(L.lib, name), ctypes._CFuncPtr), name
    for other in (L.EXPORTED, L.EXPORTED_CTX, L.EXPORTED_ACTION, L.EXPORTED_STATE16, L.EXPORTED_STORE, L.EXPORTED_SPEC,
                  L.EXPORTED_SPEC_ROOM, L.EXPORTED_SPEC_STORE, L.EXPORTED_INGEST_SEQ, L.EXPORTED_ACTION_AS):
        assert not set(L.EXPORTED_STATE_CACHE) & set(other)
    assert L.lib.simaps_abi_version() == 8 and L.lib.simaps_spec_abi_version() == 1   # the older headers are untouched
    assert L.lib.simaps_spec_room_abi_version() == 1
    assert L.has_entry('get_state_cached') and not L.has_entry('no_such_entry')


def test_cached_entry_takes_get_states_arguments_plus_the_cache(L):
    base = list(L.lib.simaps_get_state.argtypes)
    assert list(L.lib.simaps_get_state_cached.argtypes) == base + [ctypes.c_void_p, ctypes.c_int32]
    assert list(L.lib.simaps_ctx_get_state_cached.argtypes) == [ctypes.c_void_p] + base + [ctypes.c_void_p, ctypes.c_int32]
    decl = re.search(r'int simaps_get_state_cached\((.*?)\);', _header_text(), re.S).group(1)
    plain = re.search(r'int simaps_get_state\((.*?)\);', re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'simaps.h')).read(),
                                                                flags=re.S), re.S).group(1)
    names = lambda s: [a.split()[-1].lstrip('*') for a in s.replace('\n', ' ').split(',')]  # noqa: E731
    assert names(decl) == names(plain) + ['cache', 'cache_records']


def test_record_header_layout_matches_the_header(L):
    txt = _header_text()
    body = re.search(r'typedef struct simaps_state_cache_header \{(.*?)\} simaps_state_cache_header;', txt, re.S).group(1)
    fields = []
    for decl in body.split(';'):
        decl = decl.strip()
        if decl:
            ctype, rest = decl.split(None, 1)
            fields += [(ctype, n.strip()) for n in rest.split(',')]
    dt = L.STATE_CACHE_HEADER_DTYPE
    assert [n.split('[')[0] for _, n in fields] == list(dt.names)
    kinds = {'int32_t': 'i', 'uint32_t': 'u', 'float': 'f'}
    off = 0
    for ctype, n in fields:
        name = n.split('[')[0]
        count = int(n.split('[')[1].rstrip(']')) if '[' in n else 1
        assert dt.fields[name][1] == off and dt.fields[name][0].base.kind == kinds[ctype], name
        off += 4 * count
    assert off == dt.itemsize == 80
    assert dt.fields['snap_i'][1] == 48 and dt.fields['hits'][1] == 64   # 16-byte words: key x 3, results, counters


def test_record_size(L):
    c = _cfg('lifting_4-small_divider')
    h, w = c.room_h, c.room_w
    win = (h + 14) * 6 * 4
    off_free = (80 + win + 15) & ~15
    off_rec = off_free + 16 * h
    want = (off_rec + 16 + (h + 2) * ((w + 2) | 1) * 4 + 255) & ~255
    got = L.lib.simaps_state_cache_bytes(c)
    assert got == want and got % 256 == 0
    assert off_rec + L.lib.simaps_rec_cache_bytes(c) <= got + 255        # the receptacle part is a rec_cache record
    assert L.lib.simaps_state_cache_bytes(None) == L.EINVAL
    big = _cfg('pushing_4-large_empty')
    assert L.lib.simaps_state_cache_bytes(big) > got                     # any valid configuration has a size


def test_argument_checks_launch_nothing(L):
    c = _cfg('lifting_4-small_divider')
    q = L.lib.simaps_get_state_cached
    assert q(c, 0, None, None, None, None, None, None, None, 0, None, None, 8, 1) == L.EINVAL    # misaligned cache
    assert b'aligned' in L.lib.simaps_last_error()
    assert q(c, 0, None, None, None, None, None, None, None, 0, None, None, None, -1) == L.EINVAL
    assert q(c, 0, None, None, None, None, None, None, None, 0, None, None, None, 0) == 0         # N == 0: nothing to do
    assert q(None, 1, None, None, None, None, None, None, None, 0, None, None, None, 0) == L.EINVAL


def test_new_header_is_part_of_the_source_hash():
    from simaps import _srchash
    rels = [rel for rel, _ in _srchash.source_files()]
    assert 'include/simaps_state_cache.h' in rels and 'csrc/simaps_spec_cached.hip' in rels and 'csrc/state_cache.h' in rels
    mk = open(os.path.join(ROOT, 'spatial-intention-maps_amd', 'csrc', 'Makefile')).read()
    assert 'include/simaps_state_cache.h' in re.search(r'^DEPS\s*:=(.*)$', mk, re.M).group(1)
    assert 'state_cache.h' in re.search(r'^DEPS\s*:=(.*)$', mk, re.M).group(1)
    assert 'simaps_spec_cached.hip' in re.search(r'^SRCS\s*:=(.*)$', mk, re.M).group(1)


def test_state_batch_passes_the_cache_only_where_it_may(L):
    """render()'s rule, without a GPU: the keyword and the attribute, and no cache object before a render."""
    import inspect
    from simaps import batch
    assert inspect.signature(batch.StateBatch.render).parameters['state_cache'].default is None
    assert inspect.signature(batch.StateBatch.__init__).parameters['state_cache'].default is True
