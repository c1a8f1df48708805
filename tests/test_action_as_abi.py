"""CPU: the C ABI of include/simaps_action_as.h (16-bit Q maps, the exploration draw on the device) is
declared, exported and bound; its argument checks come before any device use; the older headers'
versions are untouched; and tests/explore_ref.py, the restatement of the draw the GPU tests compare
the kernels with, reproduces the published Philox4x32-10 known answers.

No kernel is launched here."""
import ctypes
import os
import re

import numpy as np
import pytest

import explore_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'simaps_action_as.h')
WANT = sorted(['simaps_action_as_abi_version', 'simaps_store_new_action_as', 'simaps_ctx_store_new_action_as'])


@pytest.fixture(scope='module')
def L():
    from simaps import _lib
    return _lib


def declared_symbols():
    """Every simaps_* name followed by `(` anywhere in the header, comments included (the rule of
    tests/test_abi.py)."""
    return sorted(set(re.findall(r'\b(simaps_[a-z_0-9]+)\s*\(', open(HEADER).read())))


def test_header_declares_exactly_the_action_as_abi(L):
    txt = open(HEADER).read()
    assert declared_symbols() == WANT
    assert '#include "simaps_action.h"' in txt and '#include "simaps_state16.h"' in txt
    assert int(re.search(r'#define SIMAPS_ACTION_AS_ABI_VERSION (\d+)', txt).group(1)) == L.ACTION_AS_ABI_VERSION == 1
    assert L.lib.simaps_action_as_abi_version() == 1
    assert L.lib.simaps_abi_version() == 8 and L.lib.simaps_action_abi_version() == 1   # the older headers' versions
    # the header states the draw: generator, the explore test, the multiply-shift and its bias, the
    # independence of the launch's agent set, and that it is not Python's stream
    for phrase in ('Philox4x32-10', '(seed & 0xffffffff, seed >> 32)', '(n, 0, step & 0xffffffff, step >> 32)',
                   '(float)(w0 >> 8) * 2^-24 < eps[n]', '(uint64_t)w1 * total >> 32', 'total / 2^32',
                   'does NOT reproduce Python'):
        assert phrase in txt, phrase


def test_library_exports_and_binds_the_action_as_abi(L):
    for name in WANT:
        assert isinstance(getattr(L.lib, name), ctypes._CFuncPtr), name
    assert sorted(L.EXPORTED_ACTION_AS) == WANT
    for other in (L.EXPORTED, L.EXPORTED_CTX, L.EXPORTED_ACTION, L.EXPORTED_STATE16, L.EXPORTED_STORE, L.EXPORTED_SPEC,
                  L.EXPORTED_INGEST_SEQ):
        assert not set(L.EXPORTED_ACTION_AS) & set(other)
    plain, twin = L.lib.simaps_store_new_action_as.argtypes, L.lib.simaps_ctx_store_new_action_as.argtypes
    assert len(plain) == 23                                     # simaps_store_new_action's 19 + q_dtype, eps, rng, out_explored
    assert plain[8] is ctypes.c_int and plain[13] is ctypes.c_int and plain[14] is ctypes.c_int   # q_dtype, flags, max_points
    assert twin[0] is ctypes.c_void_p and list(twin[1:]) == list(plain)
    # the declaration's argument list, in order
    txt = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    decl = re.search(r'int simaps_store_new_action_as\((.*?)\);', txt, flags=re.S).group(1)
    names = [re.findall(r'(\w+)\s*$', a.strip())[0] for a in decl.split(',')]
    assert names == ['cfg', 'N', 'agents', 'envs', 'robots', 'paths', 'occupancy', 'q', 'q_dtype', 'q_off', 'actions_in',
                     'eps', 'rng', 'flags', 'max_points', 'out_action', 'out_source', 'out_target', 'out_xy',
                     'out_heading', 'out_count', 'out_explored', 'stream']
    tdecl = re.search(r'int simaps_ctx_store_new_action_as\((.*?)\);', txt, flags=re.S).group(1)
    tnames = [re.findall(r'(\w+)\s*$', a.strip())[0] for a in tdecl.split(',')]
    assert tnames == ['ctx'] + names


def test_header_is_part_of_the_source_hash():
    from simaps import _srchash
    rels = [rel for rel, _ in _srchash.source_files()]
    for rel in ('include/simaps_action_as.h', 'csrc/simaps_action_as.hip', 'csrc/action_as.h', 'csrc/philox.h',
                'csrc/action_decode_body.inc', 'csrc/action_finish_body.inc'):
        assert rel in rels, rel


ARGS = ('cfg', 'N', 'agents', 'envs', 'robots', 'paths', 'occupancy', 'q', 'q_dtype', 'q_off', 'actions_in', 'eps', 'rng',
        'flags', 'max_points', 'out_action', 'out_source', 'out_target', 'out_xy', 'out_heading', 'out_count',
        'out_explored', 'stream')


def _call(L, ctx=None, twin=False, **kw):
    """simaps_store_new_action_as with plausible non-NULL dummies (never dereferenced: every call here
    must fail its argument checks first), overridden by kw."""
    from simaps import batch, constants as K
    d = ctypes.c_void_p(0x1000)
    a = dict(cfg=batch.make_config(dict(K.DEFAULT_FLAGS), 1.0, 0.5), N=1, agents=d, envs=d, robots=d, paths=d,
             occupancy=d, q=d, q_dtype=L.STATE_BF16, q_off=d, actions_in=d, eps=d, rng=d, flags=1, max_points=8,
             out_action=d, out_source=d, out_target=d, out_xy=d, out_heading=d, out_count=d, out_explored=d, stream=None)
    a.update(kw)
    args = [a[k] for k in ARGS]
    if twin:
        return L.lib.simaps_ctx_store_new_action_as(ctx, *args)
    return L.lib.simaps_store_new_action_as(*args)


@pytest.mark.parametrize('twin', [False, True], ids=['plain', 'ctx'])
def test_argument_errors_come_before_any_device_use(L, twin):
    for bad in (-1, 3, 99):
        assert _call(L, twin=twin, q_dtype=bad) == L.EINVAL, bad
        assert b'q_dtype' in L.lib.simaps_last_error()
    assert _call(L, twin=twin, rng=None) == L.EINVAL              # eps without rng
    assert b'eps without rng' in L.lib.simaps_last_error()
    # today's argument errors (tests/test_action_abi.py), through the new entry point
    for out in ('out_action', 'out_source', 'out_target', 'out_xy', 'out_heading', 'out_count'):
        assert _call(L, twin=twin, **{out: None}) == L.EINVAL, out
        assert b'NULL output' in L.lib.simaps_last_error()
    assert _call(L, twin=twin, max_points=1) == L.EINVAL
    assert b'max_points' in L.lib.simaps_last_error()
    assert _call(L, twin=twin, N=-1) == L.EINVAL
    assert _call(L, twin=twin, q_off=None) == L.EINVAL             # q without q_off
    assert b'q and q_off' in L.lib.simaps_last_error()
    assert _call(L, twin=twin, q=None) == L.EINVAL                 # q_off without q
    assert _call(L, twin=twin, q=None, q_off=None, actions_in=None) == L.EINVAL
    assert b'neither q nor actions_in' in L.lib.simaps_last_error()
    assert _call(L, twin=twin, flags=4) == L.EINVAL
    assert _call(L, twin=twin, agents=None) == L.EINVAL
    assert _call(L, twin=twin, occupancy=None) == L.EINVAL         # needed with shortest-path movement
    assert _call(L, twin=twin, paths=None, flags=3) == L.EINVAL    # needed for the write-back
    assert _call(L, twin=twin, cfg=None) == L.EINVAL
    for dt in (L.STATE_F32, L.STATE_BF16, L.STATE_F16):            # nothing to do, nothing touched (rng left alone)
        assert _call(L, twin=twin, N=0, q_dtype=dt) == 0
    assert _call(L, twin=twin, N=0, eps=None, rng=None, out_explored=None) == 0


def test_stale_context_handle_is_refused(L):
    buf = ctypes.create_string_buffer(4096)                        # live memory that is not a context
    fake = ctypes.c_void_p(ctypes.addressof(buf))
    assert _call(L, ctx=fake, twin=True) == L.EINVAL
    assert b'not a live context' in L.lib.simaps_last_error()
    assert buf.raw == b'\0' * 4096


# Known answers of Philox4x32-10 (the Random123 distribution's kat_vectors): counter, key, output
KAT = [((0, 0, 0, 0), (0, 0), '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, '408f276d 41c83b0e a20bc7c6 6d5451fd'),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
        'd16cfe09 94fdcceb 5001e420 24126ea1')]


@pytest.mark.parametrize('counter,key,want', KAT, ids=['zeros', 'ones', 'pi'])
def test_philox_restatement_reproduces_the_known_answers(counter, key, want):
    assert ' '.join('%08x' % w for w in E.philox4x32_10(counter, key)) == want


def test_draw_restatement_properties():
    """eps 1 always explores, eps 0 never; the action is inside [0, total); the draw of agent n does
    not depend on how many agents are drawn with it; the uniform is a multiple of 2^-24 below 1."""
    for n in range(64):
        assert E.draw(9, 3, n, 1.0, 9216)[0] and not E.draw(9, 3, n, 0.0, 9216)[0]
        assert 0 <= E.draw(9, 3, n, 1.0, 9216)[1] < 9216
        assert 0 <= E.draw(9, 3, n, 1.0, 18432)[1] < 18432
    ex8, a8 = E.draws(5, 2 ** 32 + 1, 8, 0.5, 18432)
    ex64, a64 = E.draws(5, 2 ** 32 + 1, 64, 0.5, 18432)
    assert np.array_equal(ex8, ex64[:8]) and np.array_equal(a8, a64[:8])
    assert E.draws(5, 1, 64, 0.5, 18432)[0].tolist() != ex64.tolist()          # the high step word counts
    assert E.draws(2 ** 32 + 5, 2 ** 32 + 1, 64, 0.5, 18432)[0].tolist() != ex64.tolist()   # and the high seed word


def test_policy_output_says_which_draw_is_which():
    """The module docstring names both ways to explore, and the step read-back says that it synchronises."""
    from simaps import policy_output
    assert 'select_actions' in policy_output.__doc__ and 'DeviceExploration' in policy_output.__doc__
    doc = policy_output.DeviceExploration.step.__doc__ + policy_output.DeviceExploration.read_step_synchronising.__doc__
    assert 'SYNCHRONIS' in doc
