"""Generate the golden vectors under tests/golden/ from the ACTUAL reference implementation.

Run in the build container only:   PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_goldens.py [which ...]
Outputs (small .npz fixtures, committed):
  c4_rules.npz   connect4 rule tables: random playouts -> valid_moves / board / win_state / observation
  c4_tree.npz    single-tree MCTS traces (find_leaf paths, per-sim root stats, counts / probs / value)
  c4_agent.npz   SelfPlayAgent lock-step self-play traces (actions, leaf-obs checksums, samples, results)
  {c4,br,tm}_edge.npz  the tree edge family (gen_edge): tests/edge_eval.py rows at PUCT ties, zero / denormal priors, exact draws,
                 configuration extremes and roots with 1, 2, 63-65 children; per-simulation paths and root rows, final records, coverage counts
  c4_mt19937.npz MCTS.search under np.random.seed(s) on numpy's own MT19937 stream: recorded child shuffles + counts / pi (second tier)
  c4_mt19937_agent.npz, br_mt19937_agent.npz   a whole SelfPlayAgent (noise + temperature on) under np.random.seed(s): every shuffle /
                 dirichlet / choice draw observed per game slot + what the agent did (connect4: 6 games; brandubh: 4 games, 53 rounds)
Every run of the reference is under the random tape (refharness.Tape) and the synthetic evaluator
(oracle azo_fake_eval), so the fixtures hold seeds + expected outputs only.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import refharness as rh  # noqa: E402
from refharness import ol  # noqa: E402

OUT = HERE


def c4_ref_to_cells(g):
    return np.asarray(g._board.pieces, dtype=np.int8).reshape(-1)


# ------------------------------------------------------------------------------------------------ rules
def gen_c4_rules(n_games=460, seed=1234):                  # >= 10^4 positions
    from alphazero.envs.connect4.connect4 import Game
    rng = np.random.RandomState(seed)
    moves, lens, valids, cells, ws, obs_crc, obs_sample = [], [], [], [], [], [], []
    for gi in range(n_games):
        g = Game()
        seq = []
        while True:
            v = np.asarray(g.valid_moves())
            w = np.asarray(g.win_state())
            valids.append(v.astype(np.uint8)); cells.append(c4_ref_to_cells(g)); ws.append(w.astype(np.uint8))
            o = g.observation()
            obs_crc.append(rh.crc(o))
            if len(obs_sample) < 64:
                obs_sample.append(o.copy())
            m = np.full(42, -1, np.int8); m[:len(seq)] = seq
            moves.append(m); lens.append(len(seq))
            if w.any():
                break
            a = int(rng.choice(np.flatnonzero(v)))
            g.play_action(a); seq.append(a)
    # Data held by the reference's own (uncollectable, old-API) test file envs/connect4/test_connect4.py,
    # re-expressed for the fixed 6x7 new API: boards are embedded bottom-left into 6x7, the expected winner stone is
    # the old test's `expected_end_state * player` (:99-151); move list -> board (:31-39); valid-move table (:58-64).
    old = [
        ([[0] * 7] * 5, 1, 0),
        ([[0, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 1, 0], [0, 0, 0, 0, 1, 0, 0], [0, 0, 0, 1, 0, 0, 0], [0, 0, 1, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0]], 1, 1),
        ([[0, 0, 0, 0, 1, 0, 0], [0, 0, 0, 1, 0, 0, 0], [0, 0, 1, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0]], -1, -1),
        ([[0, 0, 0, 0, 0, 0, 0], [0, 0, 1, 0, 0, 0, 0], [0, 0, 0, 1, 0, 0, 0], [0, 0, 0, 0, 1, 0, 0], [0, 0, 0, 0, 0, 1, 0]], -1, -1),
        ([[0, 0, 0, -1], [0, 0, -1, 0], [0, -1, 0, 0], [-1, 0, 0, 0]], 1, -1),
        ([[0, 0, 0, 0, 1], [0, 0, 0, 1, 0], [0, 0, 1, 0, 0], [0, 1, 0, 0, 0]], -1, -1),
        ([[1, 0, 0, 0, 0], [0, 1, 0, 0, 0], [0, 0, 1, 0, 0], [0, 0, 0, 1, 0]], -1, -1),
        ([[0, 0, 0, 0, 0, 0, 0], [0, 0, 0, -1, 0, 0, 0], [0, 0, 0, -1, 0, 0, 1], [0, 0, 0, 1, 1, -1, -1], [0, 0, 0, -1, 1, 1, 1], [0, -1, 0, -1, 1, -1, 1]], -1, 0),
        ([[0, 0, 0, 0, 0, 0, 0], [0, 0, 0, -1, 0, 0, 0], [1, 0, 1, -1, 0, 0, 0], [-1, -1, 1, 1, 0, 0, 0], [1, 1, 1, -1, 0, 0, 0], [1, -1, 1, -1, 0, -1, 0]], -1, -1),
        ([[0, 0, 0, 1, 0, 0, 0], [0, 0, 0, 1, 0, 0, 0], [0, 0, 0, -1, 0, 0, 0], [0, 0, 1, 1, -1, 0, -1], [0, 0, -1, 1, 1, 1, 1], [-1, 0, -1, 1, -1, -1, -1]], 1, 1),
    ]
    end_boards, end_ws, end_winner = [], [], []
    for b, player, end_state in old:
        b = np.array(b, np.int8)
        full = np.zeros((6, 7), np.int8)
        full[6 - b.shape[0]:, :b.shape[1]] = b
        g = Game(); g._board.pieces = full.astype(np.intc)
        w = np.asarray(g.win_state(), np.uint8)
        winner = end_state * player
        assert (w[0] == (winner == 1)) and (w[1] == (winner == -1)), (full, w, winner)   # reference vs its own test data
        end_boards.append(full); end_ws.append(w); end_winner.append(winner)
    end_boards = np.array(end_boards)
    g = Game()
    for a in [4, 5, 4, 3, 0, 6]:
        g.play_action(a)
    moves_board = c4_ref_to_cells(g).reshape(6, 7)
    assert (moves_board == np.array([[0] * 7] * 4 + [[0, 0, 0, 0, 1, 0, 0], [1, 0, 0, -1, 1, -1, -1]])).all()
    vm_moves = [[], [0, 1, 2, 3, 4, 5, 6], [0, 1, 2, 3, 4, 5, 6] * 5, [0, 1, 2, 3, 4, 5, 6] * 6, [0, 1, 2] * 3 + [3, 4, 5, 6] * 6]
    vm_expected = [[1] * 7, [1] * 7, [1] * 7, [0] * 7, [1] * 3 + [0] * 4]
    vm_tab = np.full((5, 42), -1, np.int8)
    for i, (mv, ex) in enumerate(zip(vm_moves, vm_expected)):
        g = Game()
        for a in mv:
            g._board.add_stone(a, 1)        # old API placed stones without win checks; valid_moves only needs occupancy
        assert list(np.asarray(g.valid_moves())) == ex
        vm_tab[i, :len(mv)] = mv
    np.savez_compressed(os.path.join(OUT, 'c4_rules.npz'), moves=np.array(moves), lens=np.array(lens, np.int16),
                        valids=np.array(valids), cells=np.array(cells), ws=np.array(ws),
                        obs_crc=np.array(obs_crc, np.uint32), obs_sample=np.array(obs_sample, np.float32),
                        end_boards=end_boards, end_ws=np.array(end_ws), end_winner=np.array(end_winner, np.int8),
                        moves_board=moves_board, vm_moves=vm_tab, vm_expected=np.array(vm_expected, np.uint8))
    print('c4_rules: %d positions' % len(lens))


# ------------------------------------------------------------------------------------------------- tree
TREE_CONFIGS = [
    # name, cpuct, fpu, noise, temp, sims
    ('default', 1.25, 0.2, False, False, 100),
    ('c4train', 4.0, 0.4, False, False, 100),
    ('noise', 1.25, 0.2, True, False, 60),
    ('noise_temp', 4.0, 0.4, True, True, 60),
]
PROB_TEMPS = [1.0, 0.5, 0.25, 0.2, 0.0]


def gen_tree(game_cls, game_id, name, n_roots, seed=7, configs=TREE_CONFIGS, max_prefix=30):
    from alphazero.MCTS import MCTS
    gi = ol.game_info(game_id)
    A, NV = gi.action_size, gi.num_players + 1
    rng = np.random.RandomState(seed)
    out = {}
    prefixes = []
    for r in range(n_roots):                  # root positions = random legal prefixes (may include none)
        g = game_cls(); seq = []
        L = 0 if r == 0 else rng.randint(0, max_prefix)
        for _ in range(L):
            v = np.flatnonzero(np.asarray(g.valid_moves()))
            a = int(rng.choice(v))
            g2 = g.clone(); g2.play_action(a)
            if np.asarray(g2.win_state()).any():
                break
            g = g2; seq.append(a)
        prefixes.append(seq)
    PL = max(len(p) for p in prefixes) + 1
    pre = np.full((n_roots, PL), -1, np.int16)
    for r, p in enumerate(prefixes):
        pre[r, :len(p)] = p
    out['prefix'] = pre
    for (cname, cpuct, fpu, noise, temp, sims) in configs:
        tape = rh.Tape(seed * 1000 + rh.crc(np.frombuffer(cname.encode(), np.uint8)) % 997)
        tape.install()
        try:
            args = rh.ref_args(game_cls, cpuct=cpuct, fpu_reduction=fpu)
            paths = np.full((n_roots, sims, 24), -1, np.int16)
            depth = np.zeros((n_roots, sims), np.int16)
            rootn = np.zeros((n_roots, sims, A), np.int16)
            rootq = np.zeros((n_roots, sims, A), np.float32)
            kmax = 128 if A > 64 else A
            fin = {k: [] for k in ('a', 'n', 'q', 'p', 'v', 'counts', 'probs', 'vmax', 'vavg', 'root_n', 'maxdepth', 'ctr')}
            for r in range(n_roots):
                g = game_cls()
                for a in prefixes[r]:
                    g.play_action(a)
                m = MCTS(args)
                tape.stream = r
                for s in range(sims):
                    leaf = m.find_leaf(g)
                    # leaf path = actions along the descent; recover from m._path + curnode
                    acts = [n.a for n in m._path[1:]] + ([m._curnode.a] if m._path else [])
                    depth[r, s] = m.depth
                    paths[r, s, :min(len(acts), 24)] = acts[:24]
                    p, v = ol.fake_eval(tape.seed, r, s, A, NV)
                    m.process_results(leaf, v, p, noise, temp)
                    for c in m._root._children:
                        rootn[r, s, c.a] = c.n; rootq[r, s, c.a] = c.q
                ch = m._root._children
                fin['a'].append(np.array([c.a for c in ch] + [-1] * (kmax - len(ch)), np.int16)[:kmax])
                fin['n'].append(np.array([c.n for c in ch] + [0] * (kmax - len(ch)), np.int32)[:kmax])
                for f in ('q', 'p', 'v'):
                    fin[f].append(np.array([getattr(c, f) for c in ch] + [0] * (kmax - len(ch)), np.float32)[:kmax])
                fin['counts'].append(np.asarray(m.counts(g)).astype(np.int32))
                fin['probs'].append(np.array([m.probs(g, t) for t in PROB_TEMPS], np.float32))
                fin['vmax'].append(m.value(False)); fin['vavg'].append(m.value(True))
                fin['root_n'].append(m._root.n); fin['maxdepth'].append(m.max_depth)
                fin['ctr'].append(tape.ctr[r])
            out[cname + '_seed'] = np.uint64(tape.seed)
            out[cname + '_cfg'] = np.array([cpuct, fpu, float(noise), float(temp), sims], np.float64)
            out[cname + '_paths'] = paths; out[cname + '_depth'] = depth
            out[cname + '_rootn'] = rootn; out[cname + '_rootq'] = rootq
            for k, v in fin.items():
                out[cname + '_' + k] = np.array(v)
        finally:
            tape.uninstall()
    out['prob_temps'] = np.array(PROB_TEMPS, np.float32)
    np.savez_compressed(os.path.join(OUT, name + '_tree.npz'), **out)
    print('%s_tree: %d roots x %s' % (name, n_roots, [c[0] for c in configs]))


def gen_c4_mt19937(n_roots=64, sims=100, seed=20250929, eval_seed=77):
    """The MT19937 tier of "identical seeds" (SURVEY.md 8c): the reference's MCTS.search on connect4 under np.random.seed(seed) with
    numpy's global legacy stream UNTOUCHED -- np.random.shuffle is observed (the real function is called, its result recorded), not
    replaced.  Per root: the recorded permutations (rank of every child, children in ascending action order, expansions concatenated
    in order), then counts / probs / root children / values.  tests/test_oracle_golden.py checks on the CPU that the recorded ranks
    ARE what np.random.RandomState(seed).shuffle produces for lists of those lengths in that order; tests/test_gpu_parity.py replays
    them on the device (azg_set_shuffle_tape)."""
    from alphazero.MCTS import MCTS
    from alphazero.envs.connect4.connect4 import Game
    A, NV = 7, 3
    rng = np.random.RandomState(4321)
    prefixes = []
    for r in range(n_roots):
        g = Game(); seq = []
        for _ in range(0 if r == 0 else rng.randint(0, 30)):
            v = np.flatnonzero(np.asarray(g.valid_moves()))
            a = int(rng.choice(v))
            g2 = g.clone(); g2.play_action(a)
            if np.asarray(g2.win_state()).any():
                break
            g = g2; seq.append(a)
        prefixes.append(seq)
    PL = max(len(p) for p in prefixes) + 1
    pre = np.full((n_roots, PL), -1, np.int16)
    for r, p in enumerate(prefixes):
        pre[r, :len(p)] = p
    args = rh.ref_args(Game, cpuct=1.25, fpu_reduction=0.2)
    real_shuffle = np.random.shuffle
    log = []

    def observed(lst):
        before = list(lst)
        real_shuffle(lst)                                   # the reference's own draw from the global MT19937 stream
        pos = [-1] * len(before)
        for new_i, obj in enumerate(lst):
            for old_i, b in enumerate(before):
                if b is obj:
                    pos[old_i] = new_i
        assert sorted(pos) == list(range(len(before)))
        log.append(pos)
    ranks, lens, fin = [], [], {k: [] for k in ('a', 'n', 'q', 'p', 'v', 'counts', 'probs1', 'probs0', 'vmax', 'vavg', 'root_n', 'maxdepth')}
    np.random.seed(seed)
    np.random.shuffle = observed
    try:
        for r in range(n_roots):
            g = Game()
            for a in prefixes[r]:
                g.play_action(a)
            m = MCTS(args)
            step = [0]

            def nn(obs, r=r, step=step):
                p, v = ol.fake_eval(eval_seed, r, step[0], A, NV)
                step[0] += 1
                return p, v
            del log[:]
            m.search(g, nn, sims, False, False)                 # MCTS.pyx:165-173
            assert step[0] == sims
            ranks.append([x for perm in log for x in perm]); lens.append([len(perm) for perm in log])
            ch = m._root._children
            fin['a'].append(np.array([c.a for c in ch] + [-1] * (A - len(ch)), np.int16))
            fin['n'].append(np.array([c.n for c in ch] + [0] * (A - len(ch)), np.int32))
            for f in ('q', 'p', 'v'):
                fin[f].append(np.array([getattr(c, f) for c in ch] + [0] * (A - len(ch)), np.float32))
            fin['counts'].append(np.asarray(m.counts(g)).astype(np.int32))
            fin['probs1'].append(np.asarray(m.probs(g, 1.0), np.float32)); fin['probs0'].append(np.asarray(m.probs(g, 0), np.float32))
            fin['vmax'].append(m.value(False)); fin['vavg'].append(m.value(True))
            fin['root_n'].append(m._root.n); fin['maxdepth'].append(m.max_depth)
    finally:
        np.random.shuffle = real_shuffle
    L = max(len(x) for x in ranks)
    tape = np.zeros((n_roots, L), np.int16)
    for r, x in enumerate(ranks):
        tape[r, :len(x)] = x
    NE = max(len(x) for x in lens)
    klen = np.zeros((n_roots, NE), np.int16)
    for r, x in enumerate(lens):
        klen[r, :len(x)] = x
    out = dict(prefix=pre, seed=np.uint64(seed), eval_seed=np.uint64(eval_seed), sims=np.int32(sims), cfg=np.array([1.25, 0.2], np.float64),
               ranks=tape, expansion_children=klen)
    for k, v in fin.items():
        out[k] = np.array(v)
    np.savez_compressed(os.path.join(OUT, 'c4_mt19937.npz'), **out)
    print('c4_mt19937: %d roots x %d sims under np.random.seed(%d), %d recorded shuffles' % (n_roots, sims, seed, sum(len(x) for x in lens)))


def gen_c4_mt19937_agent(B=4, sims=20, games=6, seed=20260929, eval_seed=91, Game=None, gid=0, name='c4'):
    """The MT19937 tier for a whole SelfPlayAgent: the reference's agent -- connect4, B concurrent games, root noise and
    root temperature ON -- plays `games` games under np.random.seed(seed) with numpy's global stream untouched; np.random.shuffle /
    dirichlet / choice / random_sample are OBSERVED (rh.ObservedRng), per game slot.  The fixture holds the global call order (kinds, slots,
    lengths: tests/test_oracle_golden.py re-derives every recorded draw from np.random.RandomState(seed) alone), the per-slot tapes in the
    engine's counter order (shuffle of k: k positions, noise event: 1, move: 1 -- azg_set_random_tape) and what the agent did: visit counts and
    sampled action per round and slot, games_played, the samples and results it queued."""
    import torch
    if Game is None:
        from alphazero.envs.connect4.connect4 import Game
    gi = ol.game_info(gid)
    A, NV = gi.action_size, gi.num_players + 1
    args = rh.ref_args(Game, numMCTSSims=sims, gamesPerIteration=games, add_root_noise=True, add_root_temp=True)
    obs = rh.ObservedRng()
    np.random.seed(seed)
    obs.install()
    rec = dict(actions=[], counts=[], games_played=[])
    try:
        ag = rh.make_ref_agent(Game, gid, B, args, obs)
        step = 0
        for rnd in range(400):
            if ag.games_played.value >= args.gamesPerIteration:
                break
            obs.stream = -1
            ag.fast = np.random.random_sample() < args.probFastSim           # SelfPlayAgent.run :84 (one coin per round)
            for s_ in range(sims):
                ag.generateBatch()
                for i in range(B):
                    p, v = ol.fake_eval(eval_seed, i, step, A, NV)
                    ag.policy_tensor[i] = torch.from_numpy(p); ag.value_tensor[i] = torch.from_numpy(v)
                ag.processBatch()
                step += 1
            rec['counts'].append([np.asarray(ag.mcts[i].counts(ag.games[i])).astype(np.int32) for i in range(B)])
            n0 = len(obs.calls)
            ag.playMoves()
            acts = [-1] * B
            for c in obs.calls[n0:]:
                if c[0] == 'choice':
                    acts[c[1]] = c[3]
            rec['actions'].append(acts)
            rec['games_played'].append(ag.games_played.value)
    finally:
        obs.uninstall()
    samples, results = ag.output_queue.items, ag.result_queue.items
    # global call order, for the RandomState check: kind (0 shuffle, 1 dirichlet, 2 choice, 3 coin), slot, length
    kinds = {'shuffle': 0, 'dirichlet': 1, 'choice': 2, 'coin': 3}
    order = np.array([[kinds[c[0]], c[1], len(c[2]) if c[0] in ('shuffle', 'dirichlet') else 1] for c in obs.calls], np.int32)
    flat_ranks = np.array([x for c in obs.calls if c[0] == 'shuffle' for x in c[2]], np.int16)
    flat_noise = np.array([x for c in obs.calls if c[0] == 'dirichlet' for x in c[2]], np.float64)
    flat_u = np.array([c[2] for c in obs.calls if c[0] in ('choice', 'coin')], np.float64)
    # per-slot tapes in the engine's counter order
    per = [[] for _ in range(B)]
    for c in obs.calls:
        if c[1] >= 0:
            per[c[1]].append(c)
    L = max(sum(len(c[2]) if c[0] == 'shuffle' else 1 for c in calls) for calls in per)
    ranks = np.zeros((B, L), np.int16); u = np.zeros((B, L), np.float64); noff = np.full((B, L), -1, np.int32); pool = []
    for sl, calls in enumerate(per):
        pos = 0
        for c in calls:
            if c[0] == 'shuffle':
                ranks[sl, pos:pos + len(c[2])] = c[2]; pos += len(c[2])
            elif c[0] == 'dirichlet':
                noff[sl, pos] = len(pool); pool.extend(np.asarray(c[2], np.float32).tolist()); pos += 1     # (:198-200 casts to float32)
            else:
                u[sl, pos] = c[2]; pos += 1
    out = dict(seed=np.uint64(seed), eval_seed=np.uint64(eval_seed), B=np.int32(B), sims=np.int32(sims), games=np.int32(games), cfg=np.array([1.25, 0.2, 0.1, 1.1], np.float64),
               call_order=order, flat_ranks=flat_ranks, flat_noise=flat_noise, flat_u=flat_u,
               tape_ranks=ranks, tape_u=u, tape_noise_off=noff, tape_noise_pool=np.array(pool, np.float32),
               actions=np.array(rec['actions'], np.int16), counts=np.array(rec['counts'], np.int32), games_played=np.array(rec['games_played'], np.int32),
               s_obs=np.array([s_[0] for s_ in samples], np.float32).reshape(len(samples), gi.obs_c, gi.obs_h, gi.obs_w),
               s_pi=np.array([s_[1] for s_ in samples], np.float32).reshape(len(samples), A),
               s_z=np.array([s_[2] for s_ in samples], np.float32).reshape(len(samples), NV),
               r_ws=np.array([np.asarray(r[1], np.uint8) for r in results]).reshape(len(results), NV),
               r_turns=np.array([r[0].turns for r in results], np.int32))
    np.savez_compressed(os.path.join(OUT, '%s_mt19937_agent.npz' % name), **out)
    nk = {k: int((order[:, 0] == v).sum()) for k, v in kinds.items()}
    print(name + '_mt19937_agent: %d slots x %d sims, %d rounds, %d games under np.random.seed(%d): %s; %d samples, %d results'
          % (B, sims, len(rec['actions']), rec['games_played'][-1], seed, nk, len(samples), len(results)))


# ------------------------------------------------------------------------------------------------ agent
AGENT_CONFIGS = [
    # name, B, sims, games, kwargs
    ('plain', 8, 25, 12, dict()),
    ('noisy', 6, 20, 8, dict(add_root_noise=True, add_root_temp=True, cpuct=4.0, fpu_reduction=0.4)),
    ('fastmix', 6, 16, 8, dict(probFastSim=0.5, numFastSims=6, symmetricSamples=False)),
    ('reset', 4, 12, 5, dict(mctsResetThreshold=3)),
    ('warmup', 6, 10, 8, dict(numWarmupSims=5)),
    ('config1', 32, 25, 32, dict()),                 # the shape of BASELINE.json configs[0]: 32 games, 25 sims
]


def run_ref_agent(game_cls, game_id, cname, B, sims, games, kw, seed, slot_base=0, is_arena=False, max_rounds=400, evaluator=None):
    import torch
    evaluator = evaluator or ol.fake_eval
    gi = ol.game_info(game_id)
    A, NV = gi.action_size, gi.num_players + 1
    is_warmup = cname == 'warmup'
    tape = rh.Tape(seed)
    tape.install()
    rec = dict(actions=[], counts=[], obs_crc=[], games_played=[], fast=[], sims=[])
    try:
        args = rh.ref_args(game_cls, numMCTSSims=sims, gamesPerIteration=games, **kw)
        ag = rh.make_ref_agent(game_cls, game_id, B, args, tape, is_arena=is_arena, is_warmup=is_warmup,
                               slot_base=slot_base)
        step = 0
        for rnd in range(max_rounds):
            if ag.games_played.value >= args.gamesPerIteration:
                break
            tape.stream = rh.AGENT_STREAM + slot_base
            ag.fast = np.random.random_sample() < args.probFastSim
            nsims = args.numFastSims if ag.fast else (args.numMCTSSims if not is_warmup else args.numWarmupSims)
            rec['fast'].append(int(ag.fast)); rec['sims'].append(nsims)
            for s in range(nsims):
                ag.generateBatch()
                if not is_warmup:
                    if is_arena:
                        data = ag.output_queue.items.pop()
                        rows = torch.cat([d for d in data if not isinstance(d, list)])
                        rec['obs_crc'].append([rh.crc(rows[i].numpy()) for i in range(B)])
                        rec.setdefault('row_game', []).append(list(ag.batch_indices))
                        for row in range(B):
                            p, v = evaluator(seed, slot_base + ag.batch_indices[row], step, A, NV)
                            ag.policy_tensor[row] = torch.from_numpy(p); ag.value_tensor[row] = torch.from_numpy(v)
                    else:
                        rec['obs_crc'].append([rh.crc(ag.batch_tensor[i].numpy()) for i in range(B)])
                        for i in range(B):
                            p, v = evaluator(seed, slot_base + i, step, A, NV)
                            ag.policy_tensor[i] = torch.from_numpy(p); ag.value_tensor[i] = torch.from_numpy(v)
                ag.processBatch()
                step += 1
            cts = []
            for i in range(B):
                m = ag.mcts[i][ag.games[i].player] if is_arena else ag.mcts[i]
                cts.append(np.asarray(m.counts(ag.games[i])).astype(np.int32))
            rec['counts'].append(cts)
            nlog = len(tape.choice_log)
            ag.playMoves()
            acts = [-1] * B
            for (st, idx) in tape.choice_log[nlog:]:
                acts[st - slot_base] = idx
            rec['actions'].append(acts)
            rec['games_played'].append(ag.games_played.value)
        samples = ag.output_queue.items if not is_arena else []
        results = ag.result_queue.items
        out = {
            'seed': np.uint64(seed), 'B': B, 'sims': sims, 'games': games,
            'actions': np.array(rec['actions'], np.int16), 'counts': np.array(rec['counts'], np.int32),
            'obs_crc': np.array(rec['obs_crc'], np.uint32).reshape(-1, B), 'games_played': np.array(rec['games_played'], np.int32),
            'fast': np.array(rec['fast'], np.int8), 'round_sims': np.array(rec['sims'], np.int32),
            's_obs': np.array([s[0] for s in samples], np.float32).reshape(len(samples), gi.obs_c, gi.obs_h, gi.obs_w),
            's_pi': np.array([s[1] for s in samples], np.float32).reshape(len(samples), A),
            's_z': np.array([s[2] for s in samples], np.float32).reshape(len(samples), NV),
            'r_ws': np.array([np.asarray(r[1], np.uint8) for r in results]).reshape(len(results), NV),
            'r_turns': np.array([r[0].turns for r in results], np.int32),
        }
        if is_arena:
            out['row_game'] = np.array(rec['row_game'], np.int32)
            out['player_to_index'] = np.array(ag.player_to_index, np.int32)
        return out, args
    finally:
        tape.uninstall()


def gen_agent(game_cls, game_id, name, configs=AGENT_CONFIGS, seed=99):
    out = {}
    for ci, (cname, B, sims, games, kw) in enumerate(configs):
        o, args = run_ref_agent(game_cls, game_id, cname, B, sims, games, kw, seed + ci, slot_base=0 if ci % 2 == 0 else 1000)
        for k, v in o.items():
            out[cname + '_' + k] = v
        out[cname + '_slot_base'] = 0 if ci % 2 == 0 else 1000
        print('  %s/%s: rounds=%d samples=%d results=%d games=%d' % (name, cname, len(o['actions']), len(o['s_pi']), len(o['r_turns']), o['games_played'][-1]))
    np.savez_compressed(os.path.join(OUT, name + '_agent.npz'), **out)


def br_game_cls():
    """The reference's brandubh Game is a cdef class without has_draw()/max_turns(): the harness adds the
    two static methods the callers need; nothing else is touched."""
    from alphazero.envs.brandubh.fastafl import Game

    class BGame(Game):
        @staticmethod
        def has_draw():
            return True

        @staticmethod
        def max_turns():
            return 100
    return BGame


def br_state(g):
    return np.asarray(g._board._state, dtype=np.int8).reshape(-1), g.player, g.turns, int(g._board._king_captured)


def gen_br_rules(n_games=170, seed=4321):                  # >= 10^4 positions
    G = br_game_cls()
    rng = np.random.RandomState(seed)
    moves, lens, valid_bits, cells, ws, kc, obs_crc, obs_sample, sym_crc, max_k = [], [], [], [], [], [], [], [], [], 0
    for gi in range(n_games):
        g = G(); seq = []
        while True:
            v = np.asarray(g.valid_moves()); w = np.asarray(g.win_state())
            c, pl, tu, k = br_state(g)
            max_k = max(max_k, int(v.sum()))
            valid_bits.append(np.packbits(v)); cells.append(c); ws.append(w.astype(np.uint8)); kc.append(k)
            o = g.observation(); obs_crc.append(rh.crc(o))
            if len(obs_sample) < 32:
                obs_sample.append(o.copy())
            m = np.full(101, -1, np.int16); m[:len(seq)] = seq
            moves.append(m); lens.append(len(seq))
            if len(seq) % 7 == 3:                      # symmetries on a subset of positions (slow in the reference)
                pi = rng.rand(588).astype(np.float32) * v
                sy = g.symmetries(pi)
                sym_crc.append([len(moves) - 1] + [rh.crc(np.asarray(st._board._state, np.float32).astype(np.int8)) ^ rh.crc(p) for st, p in sy] + [rh.crc(pi)])
            if w.any():
                break
            a = int(rng.choice(np.flatnonzero(v)))
            g.play_action(a); seq.append(a)
    np.savez_compressed(os.path.join(OUT, 'br_rules.npz'), moves=np.array(moves), lens=np.array(lens, np.int16),
                        valid_bits=np.array(valid_bits), cells=np.array(cells), ws=np.array(ws), kc=np.array(kc, np.int8),
                        obs_crc=np.array(obs_crc, np.uint32), obs_sample=np.array(obs_sample, np.float32),
                        sym_crc=np.array(sym_crc, np.int64), sym_seed=np.int64(seed), max_k=np.int32(max_k))
    print('br_rules: %d positions, max legal moves %d, %d symmetry checks' % (len(lens), max_k, len(sym_crc)))


def gen_arena(game_cls, game_id, name, B=8, sims=12, games=10, seed=555):
    """Arena-mode SelfPlayAgent traces (SelfPlayAgent.pyx:44-47,60-73,117-132,142-151,158,167-168).  The reference mis-routes
    evaluations when games desynchronise; the trace records what the reference actually does."""
    out = {}
    o, args = run_ref_agent(game_cls, game_id, 'arena', B, sims, games, dict(), seed, slot_base=0, is_arena=True)
    for k, v in o.items():
        out['arena_' + k] = v
    print('  %s/arena: rounds=%d results=%d games=%d p2i=%s' % (name, len(o['actions']), len(o['r_turns']), o['games_played'][-1], o['player_to_index']))
    np.savez_compressed(os.path.join(OUT, name + '_arena.npz'), **out)


def fill_deterministic(sd):
    """Deterministic weights from the key order, identical for the reference net and the build's net."""
    import torch
    out = {}
    for i, k in enumerate(sorted(sd)):
        t = sd[k]
        if t.dtype in (torch.int64, torch.int32):
            out[k] = t.clone()
            continue
        n = t.numel()
        x = torch.sin(torch.arange(n, dtype=torch.float64) * 0.37 + i * 1.7)
        if k.endswith('running_var'):
            x = x.abs() * 0.8 + 0.4
        elif k.endswith('running_mean') or k.endswith('.bias'):
            x = x * 0.1
        elif 'bn' in k and k.endswith('.weight'):
            x = x * 0.3 + 1.0
        else:
            x = x * (1.5 / max(t[0].numel(), 1) ** 0.5)
        out[k] = x.reshape(t.shape).to(t.dtype)
    return out


def gen_net():
    """Reference ResNet (alphazero/NNetArchitecture.py:69-120) forward on fixed boards with deterministic weights."""
    import torch
    from alphazero.NNetArchitecture import ResNet
    from alphazero.envs.connect4.connect4 import Game
    from alphazero.utils import dotdict
    out = {}
    rng = np.random.RandomState(3)
    obs = []
    for b in range(12):
        g = Game()
        for _ in range(rng.randint(0, 25)):
            v = np.flatnonzero(np.asarray(g.valid_moves()))
            if np.asarray(g.win_state()).any():
                break
            g.play_action(int(rng.choice(v)))
        obs.append(g.observation())
    obs = np.array(obs, np.float32)
    out['obs'] = obs
    for name, a in (('default', dict(num_channels=32, depth=4, value_head_channels=16, policy_head_channels=16,
                                      value_dense_layers=[512, 64], policy_dense_layers=[512, 256])),
                    ('c4train', dict(num_channels=128, depth=8, value_head_channels=32, policy_head_channels=32,
                                     value_dense_layers=[1024, 256], policy_dense_layers=[1024]))):
        net = ResNet(Game, dotdict(a))
        net.load_state_dict(fill_deterministic(net.state_dict()))
        net.eval()
        with torch.no_grad():
            lp, lv = net(torch.from_numpy(obs))
        out[name + '_policy'] = torch.exp(lp).numpy(); out[name + '_value'] = torch.exp(lv).numpy()
        out[name + '_keys'] = np.array(sorted(net.state_dict().keys()))
        out[name + '_shapes'] = np.array([str(tuple(net.state_dict()[k].shape)) for k in sorted(net.state_dict())])
    np.savez_compressed(os.path.join(OUT, 'c4_net.npz'), **out)
    print('c4_net: %d boards' % len(obs))


def gen_ckpt():
    """A checkpoint file written by the REFERENCE NNetWrapper.save_checkpoint (alphazero/NNetWrapper.py:239-250) for a tiny
    net, plus the reference's own process() outputs on fixed boards: pins load_checkpoint compatibility (keys, args, weights)."""
    import torch
    import torch.optim as optim
    from alphazero.NNetWrapper import NNetWrapper
    from alphazero.envs.connect4.connect4 import Game
    from alphazero.utils import dotdict
    torch.manual_seed(1234)
    args = dotdict(dict(nnet_type='resnet', num_channels=8, depth=2, value_head_channels=2, policy_head_channels=3,
                        value_dense_layers=[12, 6], policy_dense_layers=[10], lr=1e-2, optimizer=optim.SGD,
                        optimizer_args=dotdict(dict(momentum=0.9)), scheduler=optim.lr_scheduler.MultiStepLR,
                        scheduler_args=dotdict(dict(milestones=[10], gamma=0.1)), cuda=False, value_loss_weight=1.5))
    w = NNetWrapper(Game, args)
    w.nnet.load_state_dict(fill_deterministic(w.nnet.state_dict()))
    w.save_checkpoint(folder=OUT, filename='c4_ref_checkpoint.pth.tar')
    d = np.load(os.path.join(OUT, 'c4_net.npz'))
    w.nnet.eval()
    p, v = w.process(torch.from_numpy(d['obs']))
    np.savez_compressed(os.path.join(OUT, 'c4_ckpt.npz'), obs=d['obs'], policy=p.numpy(), value=v.numpy())
    print('c4_ckpt: %d bytes' % os.path.getsize(os.path.join(OUT, 'c4_ref_checkpoint.pth.tar')))


# ------------------------------------------------------------------------------------------------- edge family
# The tree code's edges, observed on the reference itself: exact PUCT ties, zero priors, the two forms of the seen-policy sum,
# exact draw values, cpuct / fpu / noise / temperature extremes, roots with 1, 2 and 63-65 children.  The evaluators are
# tests/edge_eval.py; every row fed is recorded as a crc.
EDGE_CONFIGS = [
    # name, evaluator family, cpuct, fpu_reduction, root noise_frac (0: off), root temperature (0: off)
    ('uniform_q', 'uniform', 0.0, 0.0, 0.0, 0.0),          # pure Q: every unvisited child ties at fpu, every visited one at q
    ('uniform_bonus', 'uniform', 1.25, -1.0, 0.0, 2.0),    # first-play bonus; root temperature 2 (numpy's ** 0.5 path)
    ('dyadic', 'dyadic', 1.25, 0.4, 0.0, 0.0),
    ('dyadic_noise1', 'dyadic', 50.0, 0.0, 1.0, 0.5),      # noise replaces the root priors; temperature 0.5 (** 2)
    ('onehot', 'onehot', 1.25, 0.4, 0.1, 0.0),
    ('onehot_q', 'onehot', 0.0, -1.0, 0.0, 2.0),
    ('spread', 'spread', 1.25, -1.0, 0.0, 0.0),            # (the bonus visits every child: wide seen-policy sums)
    ('spread_powf', 'spread', 50.0, 0.4, 0.1, 1.1),        # the powf tier
]
EDGE_PROB_TEMPS = [1.0, 2.0, 0.5, 0.1, 0.0, 0.01]          # 0.01: (counts / n) ** 100 underflows
EDGE_GAMES = {                                             # name: (game id, random roots, sims, edge root move counts)
    'c4': (ol.GAME_CONNECT4, 12, 60, (1, 2)),
    'tm': (ol.GAME_TRIMOK, 12, 48, (1, 2)),
    'br': (ol.GAME_BRANDUBH, 6, 40, (63, 64, 65)),
}
EDGE_COV = ['best_child_calls', 'tied_max', 'zero_prior_selected', 'seen_sum_tree', 'seen_sum_serial_wide', 'draw_backups', 'underflows']
EDGE_FLOORS = {                                            # per game, summed over the configs
    'tied_max': 500, 'zero_prior_selected': 50, 'seen_sum_tree': 100, 'seen_sum_serial_wide': 50, 'draw_backups': 100,
}
# The games without a C oracle (othello, gobang) register themselves here from their own generators (make_othello_goldens.py,
# make_gobang_goldens.py: `ot_edge`, `gb_edge`): name -> dict(gid, sims, game_cls(), roots(game_cls, seed) -> (roots, kinds),
# cells(g) -> the ABI cells of a reference game, agent (B, sims, games), cov [further counters], floors {counter: floor}, compact,
# extra: a second group of roots dict(prefix, sims, roots) recorded the same way under `prefix` in the same file).  Their fixtures
# carry the hook's `cov` counters (of EDGE_COV_WIDE) after those of EDGE_COV; the three oracle games' files are unchanged.
EDGE_HOOKS = {}
EDGE_COV_WIDE = [
    'chosen_chunk1', 'chosen_chunk2', 'chosen_chunk3',     # the chosen child's list index is >= 64, >= 128, >= 192
    'tie_spans_chunks',                                    # the maximal u are in at least two different chunks of 64 children
    'nc_switch',                                           # one descent selects at a node of more than 64 children, then at one of at most 64
    'zero_prior_selected_wide',                            # a zero-prior child chosen among more than 64
    'seen_sum_serial_over128',                             # seen_sum_serial_wide at a node of more than 128 children
    'noise_cast_underflows',                               # roots whose Dirichlet draw underflowed in the cast to float32 (MCTS.pyx:199-201)
]


def _edge_game_cls(name):
    if name == 'c4':
        from alphazero.envs.connect4.connect4 import Game
        return Game
    if name == 'br':
        return br_game_cls()
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from alphazero_general_amd.envs.trimok import Game
    return Game


def _ref_cells(name, g):
    if name == 'c4':
        return c4_ref_to_cells(g)
    if name == 'br':
        return br_state(g)[0]
    return np.asarray(g._board, np.int8).reshape(-1)


def _edge_roots(name, game_cls, gid, n_random, ks, seed):
    """reference game objects at the roots: random legal prefixes, then positions whose side to move has exactly k moves (found by
    playouts, or for brandubh's k > 63 -- playouts from the start stay at <= 63 -- crafted as in oracle_lib.br_wide_positions)"""
    rng = np.random.RandomState(seed)
    roots, kinds = [], []
    for r in range(n_random):
        g = game_cls()
        for _ in range(0 if r == 0 else rng.randint(0, 30)):
            v = np.flatnonzero(np.asarray(g.valid_moves()))
            g2 = g.clone(); g2.play_action(int(rng.choice(v)))
            if np.asarray(g2.win_state()).any():
                break
            g = g2
        roots.append(g); kinds.append(0)
    for k in ks:
        found = None
        for _ in range(200000 if k <= 63 else 0):          # playouts until the side to move has k moves
            o, seq = ol.OGame(gid), []
            while not o.win_state().any():
                v = np.flatnonzero(o.valid_moves())
                if len(v) == k:
                    found = seq
                    break
                a = int(rng.choice(v)); o.play(a); seq.append(a)
            if found is not None:
                break
        if found is not None:
            g = game_cls()
            for a in found:
                g.play_action(a)
        else:
            assert name == 'br'
            g = None
            for _ in range(400000):
                c = np.zeros(49, np.int8); c[[0, 6, 42, 48]] = 5; c[24] = 4
                free = np.flatnonzero(c == 0)
                pick = rng.choice(free, 9 + rng.randint(0, 3), replace=False)
                c[pick[:8]] = 2; c[pick[8]] = 3; c[pick[9:]] = 1
                st = ol.State()
                for i in range(49):
                    st.cells[i] = int(c[i])
                o = ol.OGame(gid, state=st)
                if o.win_state().any() or int(o.valid_moves().sum()) != k:
                    continue
                g = game_cls()
                g._board._state = np.array(c.reshape(7, 7), dtype=g._board._state.dtype)    # as the reference's own symmetries() does
                break
            assert g is not None, k
        assert int(np.asarray(g.valid_moves()).sum()) == k and not np.asarray(g.win_state()).any(), (name, k)
        roots.append(g); kinds.append(k)
    return roots, kinds


def _root_state(name, gid, g):
    """the oracle's state of a reference root, checked cell for cell, valid move for valid move"""
    st = ol.State()
    cells = _ref_cells(name, g)
    for i, x in enumerate(cells):
        st.cells[i] = int(x)
    st.player, st.turns = int(g.player), int(g.turns)
    if name == 'br':
        st.aux[0] = int(g._board._king_captured)
    o = ol.OGame(gid, state=st)
    assert (o.valid_moves() == np.asarray(g.valid_moves())).all() and (o.win_state() == np.asarray(g.win_state())).all(), name
    return o


def _bc_observe(nd, chosen, cpuct, fpu, cov):
    """Node.best_child (MCTS.pyx:89-104) restated in float32 over the reference's own node state, before its choice is applied:
    checks that the reference took the first maximum this computes, and counts ties, zero-prior picks and the seen-sum form the
    device takes (csrc/azg_kernels.h best_child: the reduction tree for more than six visited non-zero priors within 22 binades,
    none denormal, at most 64 children; the serial loop otherwise)"""
    import math
    ch = nd._children
    with np.errstate(all='ignore'):
        seen = 0.0
        for c in ch:
            if c.n > 0:
                seen += float(c.p)
        fpu_value = np.float32(float(np.float32(nd.v)) - float(np.float32(fpu)) * math.sqrt(float(np.float32(seen))))
        sqn = np.float32(math.sqrt(nd.n))
        cp = np.float32(cpuct)
        u = np.array([(fpu_value if c.n == 0 else np.float32(c.q)) + ((cp * np.float32(c.p)) * sqn) / np.float32(1 + c.n) for c in ch], np.float32)
    best = int(np.argmax(u))
    assert ch[best] is chosen, 'best_child restatement disagrees with the reference'
    cov['best_child_calls'] += 1
    cov['tied_max'] += int((u == u[best]).sum() > 1)
    cov['zero_prior_selected'] += int(chosen.p == 0)
    nz = np.array([c.p for c in ch if c.n > 0 and c.p != 0], np.float32)
    if len(nz) > 6:
        ex = (nz.view(np.uint32) >> 23) & 0xFF
        if len(ch) <= 64 and ex.min() > 0 and int(ex.max()) - int(ex.min()) <= 22:
            cov['seen_sum_tree'] += 1
        else:
            cov['seen_sum_serial_wide'] += 1
            if 'seen_sum_serial_over128' in cov:
                cov['seen_sum_serial_over128'] += int(len(ch) > 128)
    if 'chosen_chunk1' in cov:                              # (the games of EDGE_HOOKS: child lists of up to four chunks of 64)
        for i in (1, 2, 3):
            cov['chosen_chunk%d' % i] += int(best >= 64 * i)
        cov['tie_spans_chunks'] += int(len(set((np.flatnonzero(u == u[best]) // 64).tolist())) > 1)
        cov['zero_prior_selected_wide'] += int(chosen.p == 0 and len(ch) > 64)


def gen_edge(name, seed=31, out_dir=None, verbose=True, _group=None):
    import edge_eval as ee
    from alphazero.MCTS import MCTS
    out_dir = out_dir or OUT
    hook = EDGE_HOOKS.get(name)
    if hook is None:
        gid, n_random, sims, ks = EDGE_GAMES[name]
        game_cls = _edge_game_cls(name)
    else:
        gid, sims, game_cls = hook['gid'], (_group or hook)['sims'], hook['game_cls']()
    compact = bool(hook and hook['compact'])                # per simulation a crc of the counts row, not the root's n and q rows
    cov_names = EDGE_COV + (hook['cov'] if hook else [])
    gi = ol.game_info(gid)
    A, NV, P = gi.action_size, gi.num_players + 1, gi.num_players
    if hook is None:
        roots, kinds = _edge_roots(name, game_cls, gid, n_random, ks, seed)
        ostates = [_root_state(name, gid, g) for g in roots]
        cells = np.array([o.cells() for o in ostates], np.int8)
        aux0 = [o.s.aux[0] for o in ostates]
        root_k = [int(o.valid_moves().sum()) for o in ostates]
    else:
        roots, kinds = (_group or hook)['roots'](game_cls, seed)
        cells = np.array([hook['cells'](g) for g in roots])
        aux0 = [0] * len(roots)
        root_k = [int(np.asarray(g.valid_moves()).sum()) for g in roots]
        for g, kind, k in zip(roots, kinds, root_k):
            assert not np.asarray(g.win_state()).any() and (kind == 0 or kind == k), (name, kind, k)
    R = len(roots)
    out = dict(cells=cells, player=np.array([g.player for g in roots], np.int32),
               turns=np.array([g.turns for g in roots], np.int32), aux0=np.array(aux0, np.int32),
               root_kind=np.array(kinds, np.int32), prob_temps=np.array(EDGE_PROB_TEMPS, np.float32), sims=np.int32(sims),
               configs=np.array([c[0] for c in EDGE_CONFIGS]))
    KM = max(root_k)
    nunder, ncast, cast_pending = [0], [0], [False]

    def under(*_):
        # cast_pending is set by the Dirichlet wrapper below only when the draw holds an entry whose cast to float32 traps (tiny and
        # inexact).  _add_root_noise (MCTS.pyx:197-206) casts the draw at once and mixes it in with C floats, so the next trap IS that
        # cast; any other trap of the same process_results call is booked as an ordinary underflow.
        if cast_pending[0]:
            ncast[0] += 1
            cast_pending[0] = False
        else:
            nunder[0] += 1
    old_call = np.seterrcall(under)
    for (cname, fam, cpuct, fpu, nfrac, rtemp) in EDGE_CONFIGS:
        cov = {k: 0 for k in cov_names}
        nunder[0] = ncast[0] = 0
        noise, temp = nfrac > 0, rtemp > 0
        tape = rh.Tape(seed * 1000 + rh.crc(np.frombuffer(cname.encode(), np.uint8)) % 997)
        tape.install()
        if hook is not None:                                # (np.random.dirichlet is the tape's from here to uninstall)
            taped = np.random.dirichlet

            def dirichlet(alpha):
                x = np.asarray(taped(alpha), np.float64)
                with np.errstate(under='ignore'):
                    y = x.astype(np.float32)
                cast_pending[0] = bool(((np.abs(y) < np.finfo(np.float32).tiny) & (y.astype(np.float64) != x)).any())
                return x
            np.random.dirichlet = dirichlet
        try:
            args = rh.ref_args(game_cls, cpuct=cpuct, fpu_reduction=fpu, root_noise_frac=nfrac if noise else 0.1,
                               root_policy_temp=rtemp if temp else 1.1)
            paths = []
            depth = np.zeros((R, sims), np.int16)
            rN = np.zeros((R, sims), np.int32)
            if compact:
                cnt_crc = np.zeros((R, sims), np.uint32)
            else:
                rootn = np.zeros((R, sims, KM), np.int16); rootq = np.zeros((R, sims, KM), np.float32)
            crcs = np.zeros((R, sims), np.uint32)
            fin = {k: [] for k in ('a', 'n', 'q', 'p', 'v', 'counts', 'probs', 'probs_raised', 'vmax', 'vavg', 'root_n', 'maxdepth', 'ctr')}
            for r in range(R):
                g = roots[r]
                m = MCTS(args)
                tape.stream = r
                for s in range(sims):
                    leaf = m.find_leaf(g)
                    pn = list(m._path)
                    for i, nd in enumerate(pn):
                        _bc_observe(nd, pn[i + 1] if i + 1 < len(pn) else m._curnode, cpuct, fpu, cov)
                    if 'nc_switch' in cov and pn:           # (a child list only shrinks along a descent of these games)
                        cov['nc_switch'] += int(len(pn[0]._children) > 64 and min(len(nd._children) for nd in pn) <= 64)
                    acts = [n.a for n in pn[1:]] + ([m._curnode.a] if pn else [])
                    depth[r, s] = m.depth
                    assert len(acts) == m.depth
                    paths.append(acts)
                    term = np.asarray(leaf.win_state()).any()
                    p, v = ee.row(fam, tape.seed, r, s, A, NV, None if term else np.asarray(leaf.valid_moves()))
                    crcs[r, s] = ee.row_crc(p, v)
                    val = np.asarray(m._curnode.e, np.float32) if m._curnode.e.any() else v
                    for nd in pn:                                   # _get_value (:291-295) of every backup step
                        gv = np.float32(val[nd.player] + val[P] / np.float32(P)) if len(val) > P else val[nd.player]
                        cov['draw_backups'] += int(gv == np.float32(0.5))
                    with np.errstate(under='call'):                 # (the reference raises here)
                        m.process_results(leaf, v, p, noise, temp)
                    cast_pending[0] = False
                    ch = m._root._children
                    if compact:
                        cnt_crc[r, s] = rh.crc(np.asarray(m.counts(g)).astype(np.int32))
                    else:
                        rootn[r, s, :len(ch)] = [c.n for c in ch]; rootq[r, s, :len(ch)] = [c.q for c in ch]
                    rN[r, s] = m._root.n
                ch = m._root._children
                pad = KM - len(ch)
                fin['a'].append(np.array([c.a for c in ch] + [-1] * pad, np.int16))
                fin['n'].append(np.array([c.n for c in ch] + [0] * pad, np.int32))
                for f in ('q', 'p', 'v'):
                    fin[f].append(np.array([getattr(c, f) for c in ch] + [0] * pad, np.float32))
                fin['counts'].append(np.asarray(m.counts(g)).astype(np.int32))
                pr, raised = [], []
                for t in EDGE_PROB_TEMPS:                       # under the reference's own np.seterr(all='raise')
                    try:
                        pr.append(np.asarray(m.probs(g, t), np.float32)); raised.append(0)
                    except FloatingPointError:
                        pr.append(np.full(A, np.nan, np.float32)); raised.append(1)
                fin['probs'].append(np.array(pr)); fin['probs_raised'].append(raised)
                fin['vmax'].append(m.value(False)); fin['vavg'].append(m.value(True))
                fin['root_n'].append(m._root.n); fin['maxdepth'].append(m.max_depth)
                fin['ctr'].append(tape.ctr[r])
        finally:
            tape.uninstall()
        L = max(max(len(x) for x in paths), 1)
        pa = np.full((R * sims, L), 255, np.uint8) if compact else np.full((R * sims, L), -1, np.int16)   # (compact: actions < 255)
        for i, x in enumerate(paths):
            pa[i, :len(x)] = x
        cov['underflows'] = nunder[0]
        assert noise or ncast[0] == 0, (name, cname)
        if 'noise_cast_underflows' in cov:
            cov['noise_cast_underflows'] = ncast[0]
        else:
            assert ncast[0] == 0, (name, cname)
        if fam != 'spread':
            assert nunder[0] == 0, (name, cname)                # only the spread rows underflow
        pre = cname + '_'
        out[pre + 'seed'] = np.uint64(tape.seed)
        out[pre + 'cfg'] = np.array([cpuct, fpu, nfrac, rtemp, sims], np.float64)
        out[pre + 'family'] = np.array(fam)
        out[pre + 'paths'] = pa.reshape(R, sims, L); out[pre + 'depth'] = depth
        if compact:
            out[pre + 'counts_crc'] = cnt_crc
        else:
            out[pre + 'rootn'] = rootn; out[pre + 'rootq'] = rootq
        out[pre + 'rootN'] = rN; out[pre + 'row_crc'] = crcs
        for k, v in fin.items():
            out[pre + k] = np.array(v)
        if compact:                                         # (narrow types: child actions as uint8 with 255 for -1; edge_eval.load undoes it)
            assert A < 255 and int(depth.max()) < 256 and sims < 32768
            out[pre + 'a'] = np.where(out[pre + 'a'] < 0, 255, out[pre + 'a']).astype(np.uint8)
            out[pre + 'depth'] = depth.astype(np.uint8); out[pre + 'rootN'] = rN.astype(np.int16)
        out[pre + 'cov'] = np.array([cov[k] for k in cov_names], np.int64)
        if verbose:
            print('  %s_edge/%s: max depth %d, %s' % (name, cname, int(depth.max()), cov))
    np.seterrcall(old_call)
    out['cov_names'] = np.array(cov_names)
    if _group is not None:                                  # a further group of roots: the caller stores it under its prefix
        return ee.stack_configs(out), root_k
    tot = sum(out[c[0] + '_cov'] for c in EDGE_CONFIGS)
    for k, floor in dict(EDGE_FLOORS, **(hook['floors'] if hook else {})).items():
        assert tot[cov_names.index(k)] >= floor, (name, k, int(tot[cov_names.index(k)]), floor)
    # the agent: uniform priors, draw-heavy values, temperature 0 from the first move (np.argmax ties in the counts), symmetric samples
    aB, asims, agames = hook['agent'] if hook else ((6, 12, 6) if name != 'br' else (4, 12, 3))
    o, _ = run_ref_agent(game_cls, gid, 'edge_agent', aB, asims, agames,
                         dict(startTemp=0, temp_scaling_fn=_zero_temp), seed + 5, evaluator=ee.agent_row)
    for k, v in o.items():
        out['agent_' + k] = v
    out['agent_slot_base'] = np.int32(0)
    if compact:                                             # the observations as bit planes + plane constants, checked to decode bit for bit
        assert A < 255
        out.update(ee.pack_obs(out.pop('agent_s_obs')))
        out.update(ee.pack_pi(out.pop('agent_s_pi')))
    extra_k, extra = [], {}
    if hook and hook.get('extra'):
        sub, extra_k = gen_edge(name, seed + 1, out_dir, verbose, _group=hook['extra'])
        extra = {hook['extra']['prefix'] + k: v for k, v in sub.items()}
    if compact:                                             # (one zip entry per key, not per key and config: an entry costs ~250 bytes)
        out = ee.stack_configs(out)
    out.update(extra)
    np.savez_compressed(os.path.join(out_dir, name + '_edge.npz'), **out)
    if verbose:
        print('%s_edge: %d roots (k = %s), %d configs; agent %d rounds, %d samples; coverage %s'
              % (name, R + len(extra_k), sorted(root_k) + sorted(extra_k), len(EDGE_CONFIGS), len(o['actions']), len(o['s_pi']),
                 dict(zip(cov_names, tot.tolist()))))


def _zero_temp(cur_temp, turns, const_max_turns):
    return 0


def main():
    which = sys.argv[1:] or ['c4_rules', 'c4_tree', 'c4_agent', 'c4_arena']
    rh.import_reference()
    from alphazero.envs.connect4.connect4 import Game as C4
    if 'c4_rules' in which:
        gen_c4_rules()
    if 'c4_tree' in which:
        gen_tree(C4, ol.GAME_CONNECT4, 'c4', n_roots=64)
    if 'c4_agent' in which:
        gen_agent(C4, ol.GAME_CONNECT4, 'c4')
    if 'c4_arena' in which:
        gen_arena(C4, ol.GAME_CONNECT4, 'c4')
    if 'c4_mt19937' in which:
        gen_c4_mt19937()
    if 'c4_mt19937_agent' in which:
        gen_c4_mt19937_agent()
    if 'br_mt19937_agent' in which:                            # the same tier for the reference's second game: child lists of 40-100 moves
        gen_c4_mt19937_agent(B=4, sims=16, games=4, seed=20260930, eval_seed=93, Game=br_game_cls(), gid=ol.GAME_BRANDUBH, name='br')
    if 'c4_net' in which:
        gen_net()
    if 'c4_ckpt' in which:
        gen_ckpt()
    if 'br_rules' in which:
        gen_br_rules()
    if 'br_tree' in which:
        gen_tree(br_game_cls(), ol.GAME_BRANDUBH, 'br', n_roots=32, seed=11, max_prefix=40,
                 configs=[('default', 1.25, 0.2, False, False, 200), ('noise_temp', 1.25, 0.2, True, True, 50)])   # >= 32 roots x 200 sims
    if 'tm_tree' in which or 'tm_agent' in which:
        sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
        from alphazero_general_amd.envs.trimok import Game as TM       # the rules statement; searched by the REFERENCE MCTS
    if 'tm_tree' in which:
        gen_tree(TM, ol.GAME_TRIMOK, 'tm', n_roots=32, seed=23, max_prefix=12,
                 configs=[('default', 1.25, 0.2, False, False, 60), ('noise_temp', 2.0, 0.3, True, True, 40)])
    if 'tm_agent' in which:
        gen_agent(TM, ol.GAME_TRIMOK, 'tm', seed=777,
                  configs=[('plain', 8, 15, 12, dict()), ('noisy', 6, 10, 8, dict(add_root_noise=True, add_root_temp=True)),
                           ('wide', 32, 50, 40, dict())])
    for name in ('c4', 'tm', 'br'):
        if name + '_edge' in which or 'edge' in which:
            gen_edge(name)
    if 'br_agent' in which:
        gen_agent(br_game_cls(), ol.GAME_BRANDUBH, 'br', seed=321,
                  configs=[('plain', 6, 12, 4, dict()), ('noisy', 4, 10, 3, dict(add_root_noise=True, add_root_temp=True)),
                           ('wide', 16, 30, 10, dict()),
                           ('raw', 6, 12, 4, dict(symmetricSamples=False, probFastSim=0.5, numFastSims=6))])   # raw samples: symmetries()[6] is the identity


if __name__ == '__main__':
    main()
