"""Scripted episodes for the state cache (tests/test_state_cache_model.py on the CPU,
tests/test_gpu_state_cache_episodes.py on the GPU): 2 envs x 4 robots of the flagship, 16 steps.

An Episode owns the host scenes the oracle reads.  steps() applies each step's operations to those
scenes and yields a Step with the same operations as device commands and the step's launches; the
consumer runs the commands on a StateBatch (or not at all: nothing here needs a GPU) and calls
launch(slots) once per launch, which gives the model's outcome per slot and checks it against what
the operations themselves promise (a slot is stale from an operation that invalidates its record until
its next cached render).  Commands:

    ('set_descriptors',)                        b.set_descriptors(ep.scenes)
    ('set_descriptor_arrays',)                  b.set_descriptor_arrays(**descriptor_arrays(ep.scenes))
    ('set_maps', slots, occupancy, overhead)    b.set_maps(occupancy, overhead, slots)   (overhead may be None)
    ('ingest', slots, depth, seg)               b.ingest(depth, seg, slots=slots)

Every operation of OPS occurs in every episode (finish() asserts it), in an order the seed permutes.
"""
import numpy as np

import oracle
import state_cache_model as M
from simaps import camera, synthetic
from simaps import constants as K

FLAGSHIP = 'lifting_4-small_divider'
ENVS, ROBOTS, STEPS = 2, 4, 16
BYTE_VALUES = (0x02, 0x04, 0x08, 0x10, 0x20, 0x40, 0x80, 0xff)
OPS = ('pose_descriptors', 'pose_arrays', 'block', 'same_map', 'byte_rewrite', 'outside_flip',
       'receptacle_same_pixel', 'receptacle_new_pixel', 'robot_type', 'env_reset', 'subset_launch', 'skipped_for_steps',
       'aba_unrendered', 'aba_rendered', 'ingest', 'repeated_slot')
_SINGLE = ('pose_descriptors', 'pose_arrays', 'block', 'same_map', 'byte_rewrite', 'outside_flip',
           'receptacle_same_pixel', 'receptacle_new_pixel', 'robot_type', 'env_reset', 'ingest')
_POSE_FIELDS = ('position', 'heading', 'target_ee', 'waypoint_positions', 'waypoint_index', 'idle')


class Step:
    def __init__(self, k, unit):
        self.k, self.unit = k, unit
        self.cmds, self.launches, self.targets, self.excluded = [], [], set(), set()


class Episode:
    def __init__(self, seed):
        self.seed = seed
        self.rng = np.random.default_rng(seed)
        self._fresh = 1000 * (seed + 1)
        self.scenes = [synthetic.make_scene(FLAGSHIP, 100 * seed + e) for e in range(ENVS)]
        self.agents = [(e, a) for e in range(ENVS) for a in range(ROBOTS)]
        self.N = len(self.agents)
        self.cfg = M.config_of(self.scenes[0])
        assert M.uses_cache(self.cfg)
        self.model = M.Model(self.N, self._inputs)
        self.stale = [True] * self.N          # the slot's record (if any) does not match its inputs
        self.last_op = ['none'] * self.N
        self.seen, self.byte_values = set(), set()
        self.outcomes = {'hit': 0, 'miss': 0, 'uncached': 0}
        self.num_ops = 0
        self._skipped = [0] * self.N
        self._aba = {}
        # the plan: a cold first step, then every unit once in a seeded order (the two A -> B -> A scripts take
        # two steps each); pose_arrays comes before robot_type, because set_descriptor_arrays keeps the robot
        # classes of the batch's construction
        units = list(_SINGLE) + ['aba_unrendered', 'aba_rendered']
        units = [units[i] for i in self.rng.permutation(len(units))]
        i, j = units.index('pose_arrays'), units.index('robot_type')
        if i > j:
            units[i], units[j] = units[j], units[i]
        self.plan = ['cold']
        for u in units:
            self.plan += [u + ':B', u + ':A'] if u.startswith('aba') else [u]
        assert len(self.plan) == STEPS
        self._repeat_step = int(self.rng.integers(1, STEPS))
        self._sleeper = (int(self.rng.integers(0, self.N)), int(self.rng.integers(1, STEPS - 4)))

    # ---- the inputs of the model
    def _inputs(self, slot):
        e, a = self.agents[slot]
        return M.key(self.cfg, self.scenes[e], a), M.window_bits(self.scenes[e]['occupancy'][a], self.cfg)

    def _seed(self):
        self._fresh += 1
        return self._fresh

    def _slots_of(self, e):
        return [s for s, (ee, _) in enumerate(self.agents) if ee == e]

    def _note(self, st, name, slots, invalidates, detail=''):
        """Operation `name` touched `slots`; invalidates: one bool for all, or one per slot."""
        self.seen.add(name)
        self.num_ops += 1
        inv = [invalidates] * len(slots) if isinstance(invalidates, bool) else list(invalidates)
        for s, i in zip(slots, inv):
            self.last_op[s] = 'step %d %s%s -> %s' % (st.k, name, detail, 'miss' if i else 'hit')
            self.stale[s] = self.stale[s] or bool(i)

    def _occ(self, slot):
        e, a = self.agents[slot]
        return self.scenes[e]['occupancy'][a]

    def _upload(self, st, slot):
        st.cmds.append(('set_maps', [slot], self._occ(slot)[None].copy(), None))

    # ---- operations (each changes the host scenes and appends the device commands)
    def _pose(self, st, envs, arrays):
        for e in envs:
            other = synthetic.make_scene(FLAGSHIP, self._seed())
            for r, o in zip(self.scenes[e]['robots'], other['robots']):
                for f in _POSE_FIELDS:
                    r[f] = o[f]
                if r['type'] == 'lifting_robot':
                    r['lift_state'] = o['lift_state']
        st.cmds.append(('set_descriptor_arrays',) if arrays else ('set_descriptors',))
        self._note(st, 'pose_arrays' if arrays else 'pose_descriptors', [s for e in envs for s in self._slots_of(e)], False)

    def _block(self, st, slot):
        occ, c = self._occ(slot), self.cfg
        before = M.window_bits(occ, c)
        i, j = M.window_pixel(c, int(self.rng.integers(0, before.shape[0])), int(self.rng.integers(0, M.WIN_BYTES)))
        bh, bw = (int(x) for x in self.rng.integers(1, 7, 2))
        occ[i:min(i + bh, c.room_i0 + c.room_h + M.PAD), j:min(j + bw, M.window_a0(c) + M.WIN_BYTES)] = 1
        self._upload(st, slot)
        self._note(st, 'block', [slot], not np.array_equal(before, M.window_bits(occ, c)), ' %dx%d at (%d, %d)' % (bh, bw, i, j))

    def _same_map(self, st, slot):
        self._upload(st, slot)
        self._note(st, 'same_map', [slot], False)

    def _byte_rewrite(self, st, slot, values):
        occ, c = self._occ(slot), self.cfg
        i0, a0 = c.room_i0 - M.PAD, M.window_a0(c)
        win = occ[i0:i0 + c.room_h + 2 * M.PAD, a0:a0 + M.WIN_BYTES]      # (a view: the flagship's window is inside the map)
        for v in values:
            cand = np.argwhere((win != 0) & (win != v))
            assert len(cand), 'no nonzero byte in the window of slot %d' % slot
            r, q = cand[int(self.rng.integers(0, len(cand)))]
            win[r, q] = v
            self.byte_values.add(int(v))
        self._upload(st, slot)
        self._note(st, 'byte_rewrite', [slot], False, ' ' + ','.join('0x%02x' % v for v in values))

    def _outside_flip(self, st, slot):
        occ, c = self._occ(slot), self.cfg
        i0, a0, wh = c.room_i0 - M.PAD, M.window_a0(c), c.room_h + 2 * M.PAD
        col, row = a0 + int(self.rng.integers(0, M.WIN_BYTES)), i0 + int(self.rng.integers(0, wh))
        for i, j in ((i0 - 1, col), (i0 + wh, col), (row, a0 - 1), (row, a0 + M.WIN_BYTES)):
            occ[i, j] = 0 if occ[i, j] else 1
        self._upload(st, slot)
        self._note(st, 'outside_flip', [slot], False)

    def _receptacle(self, st, e, same_pixel):
        sc, c = self.scenes[e], self.cfg
        shape = (c.H, c.W)
        old = sc['receptacle_position']
        pi, pj = oracle.position_to_pixel_indices(old[0], old[1], shape)
        while True:
            if same_pixel:
                qi, qj = pi, pj
            else:
                qi = c.room_i0 + int(self.rng.integers(0, c.room_h))
                qj = c.room_j0 + int(self.rng.integers(0, c.room_w))
            dx, dy = self.rng.uniform(-0.4, 0.4, 2)
            new = (float(((qj + 0.5 + dx) - c.W / 2) / 96.0), float((c.H / 2 - (qi + 0.5 + dy)) / 96.0), 0)
            if new[:2] != tuple(old[:2]) and ((qi, qj) == (pi, pj)) == same_pixel:
                break
        assert oracle.position_to_pixel_indices(new[0], new[1], shape) == (qi, qj)
        sc['receptacle_position'] = new
        st.cmds.append(('set_descriptors',))
        self._note(st, 'receptacle_same_pixel' if same_pixel else 'receptacle_new_pixel', self._slots_of(e), not same_pixel,
                   ' (%d, %d) -> (%d, %d)' % (pi, pj, qi, qj))

    def _robot_type(self, st, e):
        a = int(self.rng.integers(0, ROBOTS))
        r = self.scenes[e]['robots'][a]
        assert r['type'] == 'lifting_robot' and K.cspace_radius_px('pushing_robot') != K.cspace_radius_px('lifting_robot')
        r.update(type='pushing_robot', cls=K.ROBOT_TYPES.index('pushing_robot'), lift_state='ready')
        st.cmds.append(('set_descriptors',))
        slots = self._slots_of(e)
        self._note(st, 'robot_type', slots, [self.agents[s][1] == a for s in slots], ' robot %d' % a)

    def _env_reset(self, st, e):
        new = synthetic.make_scene(FLAGSHIP, self._seed())
        slots = self._slots_of(e)
        changed = [self._inputs(s) for s in slots]
        self.scenes[e] = new
        changed = [k != self._inputs(s)[0] or not np.array_equal(b, self._inputs(s)[1]) for s, (k, b) in zip(slots, changed)]
        assert all(changed), 'a fresh scene left a slot of env %d unchanged' % e
        st.cmds.append(('set_maps', slots, new['occupancy'].copy(), new['overhead'].copy()))
        st.cmds.append(('set_descriptors',))
        self._note(st, 'env_reset', slots, True)

    def _ingest(self, st, e):
        sc, c = self.scenes[e], self.cfg
        spec = camera.CAMERAS['forward']
        robots = sorted(int(a) for a in self.rng.choice(ROBOTS, 2, replace=False))
        slots = [s for s in self._slots_of(e) if self.agents[s][1] in robots]
        depth, seg, inv = [], [], []
        for a in robots:
            db, raw = synthetic.camera_images(sc, a, 'forward', seed=self._seed())
            r = sc['robots'][a]
            before = M.window_bits(sc['occupancy'][a], c)
            oracle.ingest(sc['overhead'][a], sc['occupancy'][a], db, raw, spec.params(r['position'][0], r['position'][1], r['heading']),
                          spec, synthetic.SEG_IDS, sc['receptacle_position'] is not None)
            inv.append(not np.array_equal(before, M.window_bits(sc['occupancy'][a], c)))
            depth.append(db)
            seg.append(raw.astype(np.int32))
        st.cmds.append(('ingest', slots, np.stack(depth), np.stack(seg)))
        self._note(st, 'ingest', slots, inv)

    def _flip_one(self, st, slot):
        """One pixel of the room's inside flipped (map B of an A -> B -> A script); returns map A."""
        occ, c = self._occ(slot), self.cfg
        a = occ.copy()
        i = c.room_i0 + int(self.rng.integers(0, c.room_h))
        j = c.room_j0 + int(self.rng.integers(0, c.room_w))
        occ[i, j] = 0 if occ[i, j] else 1
        self._upload(st, slot)
        return a

    def _unit(self, st):
        u = st.unit
        e = int(self.rng.integers(0, ENVS))
        slot = int(self.rng.integers(0, self.N))
        if u == 'cold':
            return
        if u in ('pose_descriptors', 'pose_arrays'):
            envs = list(range(ENVS)) if u == 'pose_arrays' else [e]
            self._pose(st, envs, u == 'pose_arrays')
            st.targets |= {s for x in envs for s in self._slots_of(x)}
        elif u in ('block', 'same_map', 'byte_rewrite', 'outside_flip'):
            if u == 'byte_rewrite':  # three values per seed: the three seeds cover all eight
                self._byte_rewrite(st, slot, [BYTE_VALUES[(3 * self.seed + i) % len(BYTE_VALUES)] for i in range(3)])
            else:
                getattr(self, '_' + u)(st, slot)
            st.targets.add(slot)
        elif u in ('receptacle_same_pixel', 'receptacle_new_pixel'):
            self._receptacle(st, e, u == 'receptacle_same_pixel')
            st.targets |= set(self._slots_of(e))
        elif u in ('robot_type', 'env_reset', 'ingest'):
            getattr(self, '_' + u)(st, e)
            st.targets |= set(self._slots_of(e))
        elif u.endswith(':B'):  # map B; the unrendered script keeps the slot out of this step's launch
            name = u[:-2]
            was_stale = self.stale[slot]
            self._aba[name] = (slot, self._flip_one(st, slot), was_stale)
            self._note(st, name, [slot], True, ' map B')
            (st.excluded if name == 'aba_unrendered' else st.targets).add(slot)
        else:  # ':A': map A again
            name = u[:-2]
            slot, a, was_stale = self._aba.pop(name)
            self._occ(slot)[:] = a
            self._upload(st, slot)
            if name == 'aba_unrendered':  # the record still holds A (or what it held before): as if nothing happened
                self._note(st, name, [slot], False, ' map A again, B never rendered')
                self.stale[slot] = was_stale
            else:
                self._note(st, name, [slot], True, ' map A again, B was rendered')
            st.targets.add(slot)

    def _extra(self, st):
        """One more map operation on a slot the step's unit leaves alone."""
        busy = st.targets | st.excluded | {v[0] for v in self._aba.values()}
        free = [s for s in range(self.N) if s not in busy]
        if st.unit == 'cold' or not free:
            return
        slot = free[int(self.rng.integers(0, len(free)))]
        op = ('block', 'same_map', 'byte_rewrite', 'outside_flip')[int(self.rng.integers(0, 4))]
        if op == 'byte_rewrite':
            self._byte_rewrite(st, slot, [BYTE_VALUES[int(self.rng.integers(0, len(BYTE_VALUES)))]])
        else:
            getattr(self, '_' + op)(st, slot)

    def _launch_slots(self, st):
        if st.unit == 'cold':
            return list(range(self.N))
        out = set(st.excluded)
        # the sleeper: from step z0 on left out of the launches until it has missed three in a row (an
        # operation on that slot alone still renders it), then rendered
        z, z0 = self._sleeper
        keep = set(st.targets)
        if st.k >= z0 and 'skipped_for_steps' not in self.seen and z not in out:
            if self._skipped[z] < 3 and st.targets != {z}:
                out.add(z)
                keep.discard(z)
            else:
                keep.add(z)
        kind = float(self.rng.random())
        rest = [s for s in range(self.N) if s not in out and s not in keep]
        if kind < 0.5 and rest:  # a subset: drop up to three more
            drop = self.rng.choice(rest, int(self.rng.integers(1, min(3, len(rest)) + 1)), replace=False)
            out |= {int(s) for s in drop}
        slots = [s for s in range(self.N) if s not in out]
        if kind < 0.75 or out:
            slots = [slots[i] for i in self.rng.permutation(len(slots))]
        return slots

    def steps(self):
        for k, unit in enumerate(self.plan):
            st = Step(k, unit)
            self._unit(st)
            self._extra(st)
            st.launches.append(self._launch_slots(st))
            if k == self._repeat_step:  # nothing changed since the launch above: a launch that names a slot twice
                s = [int(x) for x in self.rng.choice(self.N, 3, replace=False)]
                st.launches.append([s[0], s[1], s[0], s[2]])
            yield st

    def launch(self, st, slots):
        """The model's outcomes of a cached launch of `slots`, checked against the operations' promises."""
        got = self.model.render(slots)
        for o in got:
            self.outcomes[o] += 1
        if got and got[0] == 'uncached':
            self.seen.add('repeated_slot')
            return got
        if slots != list(range(self.N)):
            self.seen.add('subset_launch')
        for s, o in zip(slots, got):
            want = 'miss' if self.stale[s] else 'hit'
            assert o == want, 'seed %d step %d slot %d: the model says %s, the operations %s (last: %s)' % (
                self.seed, st.k, s, o, want, self.last_op[s])
            self.stale[s] = False
            if self._skipped[s] >= 3:
                self.seen.add('skipped_for_steps')
        for s in range(self.N):
            self._skipped[s] = 0 if s in slots else self._skipped[s] + 1
        return got

    def finish(self):
        missing = [o for o in OPS if o not in self.seen]
        assert not missing, 'seed %d never ran %s' % (self.seed, missing)
        return {'seed': self.seed, 'hits': sum(self.model.hits), 'misses': sum(self.model.misses),
                'operations': self.num_ops, 'uncached_stacks': self.outcomes['uncached']}
