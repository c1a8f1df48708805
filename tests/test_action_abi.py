"""CPU: the action-decoding C ABI (include/simaps_action.h) is declared, exported and bound; its
argument checks come before any device use; the reference fixture tests/golden/actions.npz still
holds what the GPU tests rely on, and tests/action_ref.py restates Robot.store_new_action on it.

No kernel is launched here."""
import ctypes
import os
import re

import numpy as np
import pytest

import action_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'simaps_action.h')
WANT = sorted(['simaps_action_abi_version', 'simaps_num_output_channels', 'simaps_store_new_action',
               'simaps_ctx_store_new_action'])


@pytest.fixture(scope='module')
def L():
    from simaps import _lib
    return _lib


def declared_symbols():
    """Every simaps_* name followed by `(` anywhere in the header, comments included (the rule of
    tests/test_abi.py)."""
    return sorted(set(re.findall(r'\b(simaps_[a-z_0-9]+)\s*\(', open(HEADER).read())))


def test_header_declares_exactly_the_action_abi(L):
    txt = open(HEADER).read()
    assert declared_symbols() == WANT
    assert '#include "simaps_ctx.h"' in txt
    assert int(re.search(r'#define SIMAPS_ACTION_ABI_VERSION (\d+)', txt).group(1)) == L.ACTION_ABI_VERSION == 1
    assert L.lib.simaps_action_abi_version() == 1
    assert L.lib.simaps_abi_version() == 8                      # the two older headers' version is untouched
    flags = dict(re.findall(r'#define SIMAPS_ACTION_(SHORTEST_PATH|WRITE_BACK) (\d+)', txt))
    assert (int(flags['SHORTEST_PATH']), int(flags['WRITE_BACK'])) == (L.ACTION_SHORTEST_PATH, L.ACTION_WRITE_BACK) == (1, 2)


def test_library_exports_and_binds_the_action_abi(L):
    for name in WANT:
        assert isinstance(getattr(L.lib, name), ctypes._CFuncPtr), name
    assert sorted(L.EXPORTED_ACTION) == WANT
    assert not set(L.EXPORTED_ACTION) & set(L.EXPORTED)
    assert not set(L.EXPORTED_ACTION) & set(L.EXPORTED_CTX)
    plain, twin = L.lib.simaps_store_new_action.argtypes, L.lib.simaps_ctx_store_new_action.argtypes
    assert len(plain) == 19
    assert twin[0] is ctypes.c_void_p and list(twin[1:]) == list(plain)


def test_header_is_part_of_the_source_hash():
    from simaps import _srchash
    rels = [rel for rel, _ in _srchash.source_files()]
    assert 'include/simaps_action.h' in rels and 'csrc/action.h' in rels


def test_kernel_id(L):
    txt = open(os.path.join(ROOT, 'include', 'simaps_ctx.h')).read()
    assert '#define SIMAPS_K_ACTION 12' in txt
    assert L.K_NAMES[12] == 'action'


def test_num_output_channels(L):
    from simaps import policy_output
    f = L.lib.simaps_num_output_channels
    assert [f(t) for t in (L.LIFTING, L.PUSHING, L.THROWING, L.RESCUE)] == [2, 1, 2, 2] == A.NUM_OUTPUT_CHANNELS
    for bad in (-1, 4, 99):
        assert f(bad) == L.EINVAL
    assert policy_output.get_num_output_channels('pushing_robot') == 1
    assert policy_output.get_action_space('pushing_robot') == 9216
    assert policy_output.get_action_space('rescue_robot') == 18432
    with pytest.raises(ValueError):
        policy_output.get_num_output_channels(7)


def _call(L, ctx=None, twin=False, **kw):
    """simaps_store_new_action with plausible non-NULL dummies (never dereferenced: every call here
    must fail its argument checks first), overridden by kw."""
    from simaps import batch, constants as K
    d = ctypes.c_void_p(0x1000)
    a = dict(cfg=batch.make_config(dict(K.DEFAULT_FLAGS), 1.0, 0.5), N=1, agents=d, envs=d, robots=d, paths=d,
             occupancy=d, q=d, q_off=d, actions_in=d, flags=1, max_points=8, out_action=d, out_source=d, out_target=d,
             out_xy=d, out_heading=d, out_count=d, stream=None)
    a.update(kw)
    args = [a[k] for k in ('cfg', 'N', 'agents', 'envs', 'robots', 'paths', 'occupancy', 'q', 'q_off', 'actions_in',
                           'flags', 'max_points', 'out_action', 'out_source', 'out_target', 'out_xy', 'out_heading',
                           'out_count', 'stream')]
    if twin:
        return L.lib.simaps_ctx_store_new_action(ctx, *args)
    return L.lib.simaps_store_new_action(*args)


@pytest.mark.parametrize('twin', [False, True], ids=['plain', 'ctx'])
def test_argument_errors_come_before_any_device_use(L, twin):
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
    assert _call(L, twin=twin, N=0) == 0                           # nothing to do, nothing touched


def test_stale_context_handle_is_refused(L):
    buf = ctypes.create_string_buffer(4096)                        # live memory that is not a context
    fake = ctypes.c_void_p(ctypes.addressof(buf))
    assert _call(L, ctx=fake, twin=True) == L.EINVAL
    assert b'not a live context' in L.lib.simaps_last_error()
    assert buf.raw == b'\0' * 4096


def test_fixture_integrity():
    cases = A.load_cases()
    non_straight = [c for c in cases if len(c['path']) > 2]
    backup = [c for c in non_straight if not np.array_equal(c['path'][-2], c['wp'][-2])]
    assert len(non_straight) >= 600 and len(backup) >= 80, (len(non_straight), len(backup))
    ks = {A.NUM_OUTPUT_CHANNELS[c['type']] for c in cases}
    assert ks == {1, 2}
    assert {c['type'] for c in cases} == {0, 1, 2, 3}
    assert sum('wp_nospm' in c for c in cases) >= 7 * 3
    assert max(len(c['path']) for c in cases) <= 16               # SIMAPS_MAX_PATH
    for c in cases:
        assert len(c['path']) == len(c['wp']) == len(c['hd']) >= 2
        assert np.array_equal(c['path'][0], c['wp'][0])           # the source is never moved


def test_numpy_restatement_reproduces_every_fixture_case():
    """tests/action_ref.py vs the reference's own outputs, on the fixture's own pre-offset path: the
    tuple exact; target, waypoints and headings to 1e-12 (same host libm class: in practice 0)."""
    from simaps import synthetic
    scenes = {}
    worst = 0.0
    for c in A.load_cases():
        key = (c['config'], c['seed'])
        if key not in scenes:
            scenes[key] = A.make_scene(synthetic, *key)
        r = scenes[key]['robots'][c['agent']]
        assert A.TYPE_IDS[r['type']] == c['type']
        assert A.action_tuple(c['action'], c['type']) == c['tuple']
        t = A.target(c['action'], c['type'], r['position'], r['heading'])
        wp, hd, _ = A.finish(c['path'], c['type'], r['heading'])
        assert np.array_equal(c['path'][0], np.asarray(r['position'][:2], dtype=np.float64))
        assert np.array_equal(c['path'][-1], c['target'])
        err = max(np.abs(np.asarray(t) - c['target']).max(), np.abs(wp - c['wp']).max(), A.angle_diff(hd, c['hd']).max())
        worst = max(worst, float(err))
        if 'wp_nospm' in c:
            wp2, hd2, _ = A.finish(np.stack([c['path'][0], c['target']]), c['type'], r['heading'])
            worst = max(worst, float(np.abs(wp2 - c['wp_nospm']).max()), float(A.angle_diff(hd2, c['hd_nospm']).max()))
    assert worst <= 1e-12, worst


def test_select_actions_follows_the_reference_draws():
    """policies.py:61-62: one random() per robot, a randrange over the action space after each hit."""
    import random
    import torch
    from simaps import policy_output
    big = [(list(range(6)), torch.zeros(6, 2, 96, 96)), (list(range(5)), torch.zeros(5, 1, 96, 96))]
    rng, ref = random.Random(5), random.Random(5)
    got = policy_output.select_actions(big, 0.5, rng)
    want = [[(ref.randrange(k * 9216) if ref.random() < 0.5 else -1) for _ in range(n)] for n, k in ((6, 2), (5, 1))]
    outputs = [([0, 2], torch.zeros(2, 2, 96, 96)), ([1], torch.zeros(1, 1, 96, 96)), ([], None)]
    assert got == want and any(a >= 0 for g in got for a in g) and any(a == -1 for g in got for a in g)
    assert policy_output.select_actions(outputs, 0.0, random.Random(1)) == [[-1, -1], [-1], []]
    full = policy_output.select_actions(outputs, 0.0, random.Random(1), group_sizes=[3, 2, 1])
    assert full == [[-1, None, -1], [None, -1], [None]]
