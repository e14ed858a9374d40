"""The defender's half of the forced-win solver (omok_env_vcf_defend) and the report built on it (records.GameRecords.vcf_defence),
restated in plain Python from the rule in include/omok_mi355x.h (a helper of tests/test_vcf_defence.py and tests/test_gpu_vcf_defence.py;
not a test, no product code).

The rule is a plain loop over vcf_solver.solve and the oracle's FIVE (vcf_solver.fives, which goes through threat_opponent.five): no cell is
skipped, whatever the null move says.

  defend(n, board, me, D, NB)              -> Map(status, moves, nodes, reply [HW], threat (verdict, moves, cell))
  defend_batch(n, boards, turns, D, NB)    -> what Engine.env_vcf_defend returns, as a dict
  report(n, start, cells, status, D, NB)   -> one game of the report, walked move by move
  set_a(n) / set_b(n), want(tag, n, D, NB) -> the shared test sets and their yardstick results, computed once per process
"""
import collections
import ctypes as C

import numpy as np

from oracle import oracle as O
import scripted_opponent as SO
import threat_opponent as TO
import vcf_solver as VS

OCCUPIED, SAFE, WINS, LOSES, UNKNOWN = 0, 1, 2, 3, 4  # OMOK_VCFD_*
_STATUS_OF_VERDICT = {0: SAFE, 1: LOSES, -1: UNKNOWN}

Map = collections.namedtuple("Map", "status moves nodes reply threat")


def defend(n, board, me, D, NB):
    board = [int(s) if int(s) in (O.BLACK, O.WHITE) else O.EMPTY for s in board]  # a byte other than 1 or 2 counts as empty
    hw = n * n
    r0 = VS.solve(n, board, 1 - me, D, NB)
    wins = set(VS.fives(n, board, me))
    status, moves, nodes, reply = [OCCUPIED] * hw, [0] * hw, [0] * hw, [-1] * hw
    for a in range(hw):
        if board[a] != O.EMPTY:
            continue
        if a in wins:
            status[a] = WINS
            continue
        board[a] = TO.stone_of(me)
        r = VS.solve(n, board, 1 - me, D, NB)
        board[a] = O.EMPTY
        status[a], moves[a], nodes[a], reply[a] = _STATUS_OF_VERDICT[r.verdict], r.moves, r.nodes, r.cell
    return Map(status, moves, nodes, reply, (r0.verdict, r0.moves, r0.cell))


def counts(status):
    status = np.asarray(status).reshape(len(status), -1)
    return {name: np.count_nonzero(status == v, axis=1).astype(np.int32) for name, v in (("safe", SAFE), ("wins", WINS), ("loses", LOSES), ("unknown", UNKNOWN))}


def defend_batch(n, boards, turns, D, NB):
    """the dict of Engine.env_vcf_defend: status, moves uint8 [B][HW]; nodes, reply int32 [B][HW]; threat int32 [B][3]; safe, wins, loses, unknown [B]"""
    maps = [defend(n, b, int(t), D, NB) for b, t in zip(boards, turns)]
    hw = n * n
    out = {"status": np.array([m.status for m in maps], dtype=np.uint8).reshape(len(maps), hw),
           "moves": np.array([m.moves for m in maps], dtype=np.uint8).reshape(len(maps), hw),
           "nodes": np.array([m.nodes for m in maps], dtype=np.int32).reshape(len(maps), hw),
           "reply": np.array([m.reply for m in maps], dtype=np.int32).reshape(len(maps), hw),
           "threat": np.array([m.threat for m in maps], dtype=np.int32).reshape(len(maps), 3)}
    out.update(counts(out["status"]))
    return out


KEYS = ("status", "moves", "nodes", "reply", "threat", "safe", "wins", "loses", "unknown")


# ---- the shared test sets ---------------------------------------------------------------------------------------------------------
def hand_set(n):
    """(names, boards, turns) of vcf_solver.hand_made(n), in name order, each with its own side to move"""
    hand = sorted(VS.hand_made(n).items())
    return ([name for name, _v in hand], np.stack([b for _name, (b, _s, _d, _w) in hand]),
            np.array([s for _name, (_b, s, _d, _w) in hand], dtype=np.uint8))


def _set(n, stride):
    _names, hb, ht = hand_set(n)
    rb, rt = VS.random_set(n)
    return np.concatenate([hb, rb[::stride]]), np.concatenate([ht, rt[::stride]])


def set_a(n):
    return _set(n, 7)


def set_b(n):
    return _set(n, 11)


_SETS = {"a": set_a, "b": set_b, "hand": lambda n: hand_set(n)[1:]}
_WANT = {}


def want(tag, n, D, NB):
    """defend_batch on set_a ("a"), set_b ("b") or the hand-made positions alone ("hand"): computed once per process and left unchanged"""
    if (tag, n, D, NB) not in _WANT:
        boards, turns = _SETS[tag](n)
        _WANT[(tag, n, D, NB)] = defend_batch(n, boards, turns, D, NB)
    return _WANT[(tag, n, D, NB)]


# ---- the report of records.GameRecords.vcf_defence, walked game by game --------------------------------------------------------------
NAMES = ("threatened", "defensible", "held", "conceded", "unknown")


def report(n, start, cells, status, D, NB):
    """One game: (threat_before of every move, {name: [2]} for NAMES).  In front of move p, with the mover `side` to move: stage 1 is
    solve for the OTHER side (threat_before[p] = its moves, 0 none, -1 budget: that counts as unknown); stage 2, where that is a win in
    m >= 2, is defend: threatened; defensible if some cell is WINS or SAFE; then held / conceded by the played cell's status (WINS or SAFE
    / LOSES); the played cell UNKNOWN counts as unknown."""
    start = np.asarray(start, dtype=np.uint8).reshape(-1)
    env = SO.make_env(n, start, int(np.count_nonzero(start)) & 1)
    before = []
    out = {name: [0, 0] for name in NAMES}
    for i, cell in enumerate(cells):
        side = int(env.turn)
        board = [int(env.board[a]) for a in range(n * n)]
        r = VS.solve(n, board, 1 - side, D, NB)
        before.append(r.moves if r.verdict == 1 else r.verdict)
        if r.verdict < 0:
            out["unknown"][side] += 1
        if r.verdict == 1 and r.moves >= 2:
            m = defend(n, board, side, D, NB)
            assert m.threat == (r.verdict, r.moves, r.cell)
            way_out = any(s in (WINS, SAFE) for s in m.status)
            at = m.status[int(cell)]
            assert at != OCCUPIED
            out["threatened"][side] += 1
            out["defensible"][side] += way_out
            out["held"][side] += way_out and at in (WINS, SAFE)
            out["conceded"][side] += way_out and at == LOSES
            out["unknown"][side] += at == UNKNOWN
        assert O.lib().orc_env_place_stone(C.byref(env), int(cell)) == (O.IN_PROGRESS if i + 1 < len(cells) else status)
    return before, {name: [int(x) for x in v] for name, v in out.items()}
