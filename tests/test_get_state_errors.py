"""CPU: what the eight get_state entry points answer to bad arguments -- the return code and the text of
simaps_last_error() -- for simaps_get_state, _cached, _as, _as_cached, _into, _into_cached, _mixed and
_mixed_as, each as simaps_<name> and as simaps_ctx_<name> on the default context (ctx NULL).  These are
the checks a call walks through ahead of its launch (check_state_cache, check_state_as, check_state_into,
then get_state_impl / get_state_mixed_impl up to N == 0 or the NULL-buffer test in simaps.hip), so they pin
what a change to that plumbing must keep.  The expected codes and texts were recorded from the library
as it was before the launchers took a descriptor (csrc/get_state_launch.h).

No kernel is launched and no device is touched: every call here returns before pending_faults."""
import pytest

F32, BF16, F16 = 0, 1, 2
FLAGSHIP = 'lifting_4-small_divider'
ODD = 8          # a pointer that is not 16-byte aligned (never dereferenced)
SOME = 4096      # an aligned non-NULL pointer (never dereferenced)
ENTRIES = ['get_state', 'get_state_cached', 'get_state_as', 'get_state_as_cached', 'get_state_into',
           'get_state_into_cached', 'get_state_mixed', 'get_state_mixed_as']
TYPED = [e for e in ENTRIES if e.endswith('_as') or '_as_' in e or '_into' in e]     # take a state_dtype
AS = [e for e in ENTRIES if e.endswith('_as') or '_as_' in e]                         # check the state's alignment
INTO = [e for e in ENTRIES if '_into' in e]
CACHED = [e for e in ENTRIES if e.endswith('_cached')]
BOTH = [False, True]                                                                  # simaps_<name>, simaps_ctx_<name>


@pytest.fixture(scope='module')
def L():
    from simaps import _lib
    return _lib


@pytest.fixture(scope='module')
def cfg():
    from simaps import batch, constants as K, synthetic
    length, width, _ = K.room_dims(synthetic.CONFIGS[FLAGSHIP]['env_name'])
    return batch.make_config(synthetic.config_flags(FLAGSHIP), width, length, 'chw', 'fma')


def call(L, entry, ctx, cfg, N=0, state=None, dtype=BF16, capacity=0, dest=None, cache=None, records=0):
    """entry(...) with every input buffer NULL and the named arguments where the entry has them; returns
    (code, last error)."""
    six = (None,) * 6                                                    # agents, envs, robots, paths, occupancy, overhead
    if 'mixed' in entry:
        # cfgs, num_robots_per_env, n_cfgs, N, agents, agent_cfg, envs, robots, paths, occupancy, map_off, overhead,
        # state, out_off[, state_dtype], stream
        args = (cfg, None, 1, N) + (None,) * 8 + (state, None) + ((dtype,) if entry.endswith('_as') else ()) + (None,)
    else:
        args = (cfg, N) + six + (state,)
        if entry in TYPED:
            args += (dtype,)
        if entry in INTO:
            args += (capacity, dest)
        args += (0, None, None)                                          # num_robots_per_env, dbg, stream
        if entry in CACHED:
            args += (cache, records)
    fn = getattr(L.lib, ('simaps_ctx_' if ctx else 'simaps_') + entry)
    rc = fn(*(((None,) if ctx else ()) + args))
    return rc, L.lib.simaps_last_error().decode()


@pytest.mark.parametrize('ctx', BOTH)
@pytest.mark.parametrize('entry', ENTRIES)
def test_no_agents_is_no_work_with_every_buffer_null(L, cfg, entry, ctx):
    for dt in (F32, BF16, F16):
        assert call(L, entry, ctx, cfg, N=0, dtype=dt)[0] == 0


@pytest.mark.parametrize('ctx', BOTH)
@pytest.mark.parametrize('entry', TYPED)
def test_unknown_state_dtype(L, cfg, entry, ctx):
    for dt in (-1, 3):
        for n in (0, 1):                                                 # refused whatever N is
            assert call(L, entry, ctx, cfg, N=n, dtype=dt, state=SOME, dest=SOME) == \
                (L.EINVAL, 'unknown state_dtype %d (SIMAPS_STATE_F32, _BF16 or _F16)' % dt)


@pytest.mark.parametrize('ctx', BOTH)
@pytest.mark.parametrize('entry', AS)
def test_misaligned_state(L, cfg, entry, ctx):
    for dt in (F32, BF16, F16):
        assert call(L, entry, ctx, cfg, N=1, dtype=dt, state=ODD) == (L.EINVAL, 'state 0x8 is not aligned to 16 bytes')
    assert call(L, entry, ctx, cfg, N=1, state=None) == (L.EINVAL, 'state is NULL')
    assert call(L, entry, ctx, cfg, N=0, state=ODD)[0] == 0              # no agents: the state is not looked at


@pytest.mark.parametrize('ctx', BOTH)
@pytest.mark.parametrize('entry', INTO)
def test_store_capacity_and_dest(L, cfg, entry, ctx):
    for dt in (F32, BF16, F16):
        assert call(L, entry, ctx, cfg, N=1, dtype=dt, state=ODD, capacity=4, dest=SOME) == \
            (L.EINVAL, 'store 0x8 is not aligned to 16 bytes')
        assert call(L, entry, ctx, cfg, N=1, dtype=dt, state=SOME, capacity=-1, dest=SOME) == (L.EINVAL, 'capacity -1 < 0')
        assert call(L, entry, ctx, cfg, N=0, dtype=dt, capacity=-1) == (L.EINVAL, 'capacity -1 < 0')
        assert call(L, entry, ctx, cfg, N=1, dtype=dt, state=SOME, capacity=4, dest=None) == (L.EINVAL, 'dest is NULL')
    assert call(L, entry, ctx, cfg, N=1, state=None, capacity=4, dest=SOME) == (L.EINVAL, 'store is NULL')
    # an empty store may be NULL or odd; the call then stops at its NULL input buffers
    assert call(L, entry, ctx, cfg, N=1, state=ODD, capacity=0, dest=SOME) == (L.EINVAL, 'NULL buffer')
    assert call(L, entry, ctx, cfg, N=1, state=None, capacity=0, dest=SOME) == (L.EINVAL, 'NULL buffer')


@pytest.mark.parametrize('ctx', BOTH)
@pytest.mark.parametrize('entry', CACHED)
def test_cache_alignment_and_records(L, cfg, entry, ctx):
    for n in (0, 1):
        assert call(L, entry, ctx, cfg, N=n, state=SOME, dest=SOME, cache=ODD, records=1) == \
            (L.EINVAL, 'cache 0x8 is not aligned to 16 bytes')
        assert call(L, entry, ctx, cfg, N=n, state=SOME, dest=SOME, cache=SOME, records=-1) == \
            (L.EINVAL, 'cache_records -1 < 0')
    assert call(L, entry, ctx, cfg, N=0, cache=SOME, records=4)[0] == 0
    assert call(L, entry, ctx, cfg, N=0, cache=None, records=4)[0] == 0
    if entry != 'get_state_cached':                                      # the cache is checked ahead of the element type
        assert call(L, entry, ctx, cfg, dtype=7, cache=ODD, records=1)[1] == 'cache 0x8 is not aligned to 16 bytes'
        assert call(L, entry, ctx, cfg, dtype=7, cache=SOME, records=1)[1] == \
            'unknown state_dtype 7 (SIMAPS_STATE_F32, _BF16 or _F16)'


@pytest.mark.parametrize('ctx', BOTH)
@pytest.mark.parametrize('entry', ENTRIES)
def test_the_checks_get_state_impl_makes_ahead_of_a_launch(L, cfg, entry, ctx):
    mixed = 'mixed' in entry
    assert call(L, entry, ctx, cfg, N=-1) == (L.EINVAL, 'N < 0')
    assert call(L, entry, ctx, None, N=0) == (L.EINVAL, 'n_cfgs 1 not in [1, 8]' if mixed else 'cfg is NULL')
    # N > 0 and a state to write, but no inputs
    assert call(L, entry, ctx, cfg, N=1, state=SOME, capacity=4, dest=SOME) == (L.EINVAL, 'NULL buffer')
    bad = type(cfg).from_buffer_copy(cfg)
    bad.rotate_rounding = 5
    assert call(L, entry, ctx, bad, N=0) == (L.EINVAL, 'bad rotate_rounding 5')
    bad = type(cfg).from_buffer_copy(cfg)
    bad.room_w = bad.W + 1
    assert call(L, entry, ctx, bad, N=1, state=SOME, dest=SOME) == (L.EINVAL, 'room rect outside the grid')
