"""CPU: which room class the get_state instances take, through the C ABI
(include/simaps_spec_room.h: simaps_get_state_room_class) -- declared, exported, bound, part of the
source hash; the small room for every small_* configuration that takes S1 / S2, none for a shape that
differs in one cell, for the large rooms, for the generic kernel's configurations and for a call with
a debug output.  simaps_get_state_instance's own answers (tests/test_spec_abi.py) are untouched.

No kernel is launched here."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'simaps_spec_room.h')
WANT = sorted(['simaps_spec_room_abi_version', 'simaps_get_state_room_class'])
NONE, SMALL = 0, 1
SHAPE_FIELDS = ('H', 'W', 'room_h', 'room_w')


@pytest.fixture(scope='module')
def L():
    from simaps import _lib
    return _lib


def _cfg(name, layout='chw', rounding='fma'):
    from simaps import batch, constants as K, synthetic
    length, width, _ = K.room_dims(synthetic.CONFIGS[name]['env_name'])
    return batch.make_config(synthetic.config_flags(name), width, length, layout, rounding)


def test_header_declares_exactly_the_query(L):
    txt = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r'\b(simaps_[a-z_0-9]+)\s*\(', txt))) == WANT == sorted(L.EXPORTED_SPEC_ROOM)
    assert int(re.search(r'#define SIMAPS_SPEC_ROOM_ABI_VERSION (\d+)', txt).group(1)) == L.SPEC_ROOM_ABI_VERSION
    assert L.lib.simaps_spec_room_abi_version() == L.SPEC_ROOM_ABI_VERSION
    for name, val in (('NONE', L.ROOM_NONE), ('SMALL', L.ROOM_SMALL)):
        assert int(re.search(r'#define SIMAPS_ROOM_%s (\d+)' % name, txt).group(1)) == val
    assert (L.ROOM_NONE, L.ROOM_SMALL) == (NONE, SMALL)
    shape = tuple(int(re.search(r'#define SIMAPS_ROOM_SMALL_%s (\d+)' % f, txt).group(1)) for f in ('H', 'W', 'RH', 'RW'))
    assert shape == L.ROOM_SMALL_SHAPE
    for name in WANT:
        assert isinstance(getattr(L.lib, name), ctypes._CFuncPtr), name
    for other in (L.EXPORTED, L.EXPORTED_CTX, L.EXPORTED_ACTION, L.EXPORTED_STATE16, L.EXPORTED_STORE, L.EXPORTED_SPEC,
                  L.EXPORTED_INGEST_SEQ, L.EXPORTED_ACTION_AS):
        assert not set(L.EXPORTED_SPEC_ROOM) & set(other)
    assert L.lib.simaps_spec_abi_version() == 1 and L.lib.simaps_abi_version() == 8     # the older headers are untouched


def test_new_header_is_part_of_the_source_hash():
    from simaps import _srchash
    assert 'include/simaps_spec_room.h' in [rel for rel, _ in _srchash.source_files()]
    mk = open(os.path.join(ROOT, 'spatial-intention-maps_amd', 'csrc', 'Makefile')).read()
    assert 'include/simaps_spec_room.h' in re.search(r'^DEPS\s*:=(.*)$', mk, re.M).group(1)


def test_small_room_shape_is_the_small_configurations_own(L):
    c = _cfg('lifting_4-small_divider')
    assert tuple(getattr(c, f) for f in SHAPE_FIELDS) == L.ROOM_SMALL_SHAPE
    assert ((c.room_w + 2) | 1) == 95 and c.room_h <= 63            # pitch 95, one cell per lane on the column sweeps


def test_every_shipped_configuration_has_its_room_class(L):
    from simaps import synthetic
    q, inst = L.lib.simaps_get_state_room_class, L.lib.simaps_get_state_instance
    seen = set()
    for name, conf in synthetic.CONFIGS.items():
        small = conf['env_name'].startswith('small')
        for rounding in ('fma', 'plain'):
            c = _cfg(name, rounding=rounding)
            spec = inst(c, 0)
            want = SMALL if small and spec != L.SPEC_GENERIC else NONE
            assert q(c, 0) == want, (name, rounding)
            assert q(c, 1) == NONE, name                                 # a debug output: the generic kernel
            assert q(_cfg(name, 'hwc'), 0) == NONE, name                 # the instances are CHW
            seen.add((spec, want))
    assert {(L.SPEC_S1, SMALL), (L.SPEC_S2, SMALL), (L.SPEC_S1, NONE), (L.SPEC_GENERIC, NONE)} <= seen
    assert q(None, 0) == L.EINVAL


@pytest.mark.parametrize('name, spec', [('lifting_4-small_divider', 1), ('rescue_4-small_empty', 2)])
def test_one_cell_off_takes_the_plain_instance(L, name, spec):
    q, inst = L.lib.simaps_get_state_room_class, L.lib.simaps_get_state_instance
    assert q(_cfg(name), 0) == SMALL
    for f in SHAPE_FIELDS:
        for d in (-1, 1):
            c = _cfg(name)
            setattr(c, f, getattr(c, f) + d)
            assert q(c, 0) == NONE, (f, d)
            assert inst(c, 0) == spec, (f, d)                            # S1 / S2 as before
    # what a class does not fix does not matter: the origin, thickness, encodings, scales
    c = _cfg(name)
    c.room_i0, c.room_j0, c.intention_map_encoding, c.intention_map_line_thickness = 60, 64, 3, 1
    c.shortest_path_map_scale, c.intention_map_scale = 0.5, 2.0
    assert q(c, 0) == SMALL and inst(c, 0) == spec
    # has_debug by truthiness, as simaps_get_state_instance takes it
    assert q(_cfg(name), 2) == q(_cfg(name), -1) == NONE


def test_state_batch_reports_the_room_class_beside_the_instance(L):
    from simaps import batch
    c = _cfg('lifting_4-small_divider')

    class B:  # the fields kernel_instance / room_class read
        cfg, flags, _rec = c, {'use_shortest_path_to_receptacle_map': True}, None
    room, inst = batch.StateBatch.room_class, batch.StateBatch.kernel_instance
    assert (inst(B), room(B)) == (L.SPEC_S1, SMALL)
    assert room(B, debug={}) == SMALL and room(B, debug={'status': None}) == SMALL
    assert room(B, debug=True) == NONE and room(B, debug={'status': object()}) == NONE
    B._rec = object()
    assert (inst(B), room(B)) == (L.SPEC_GENERIC, NONE)
