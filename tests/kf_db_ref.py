"""Restatement of KeyFrameDatabase (src/KeyFrameDatabase.cc:40-73 add / erase / clear, :76-197 DetectLoopCandidates, :199-309
DetectRelocalizationCandidates) and of the vocabulary's score functions (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-310) in plain Python,
written from reading them.  It is the reference's SHAPE, not the device's: a literal inverted file (a list of key frames per word, in
add order) that the query walks word by word, and per key frame the query / words / score fields the walk leaves behind.  The order of the
candidates therefore comes out of the walk, and the device's claim that this order is (smallest common word, order of add) is tested, not
assumed.  Python floats are the reference's doubles, np.float32 its floats.

Defined where the reference is not (the library's DEFINED BEHAVIOUR): a key frame's two scores start at 0.0f (KeyFrame.cc:36 leaves them
uninitialised); an erased key frame takes part in nothing, also not as a neighbour; a neighbour that is not in the database is skipped.

Also the generators of the random databases and the crafted cases tests/test_kf_db.py checks on the CPU and tests/test_kf_db_gpu.py runs on
the device.  A case is a SCRIPT: a list of operations ("add", slot, words, values) / ("erase", slot) / ("clear",) / ("cov", slot, slots) /
("query", words, values, mode, min_score, connected) that run_script plays on anything with those methods."""
import bisect
import math

import numpy as np

L1_NORM, L2_NORM, CHI_SQUARE, KL, BHATTACHARYYA, DOT_PRODUCT = 0, 1, 2, 3, 4, 5
RELOC, LOOP = 0, 1
F32 = np.float32


# ------------------------------------------------------------------------------------------------ score()
def score(scoring, w1, v1, w2, v2):
    """the double the scoring object returns for v1 (the query) and v2 (the key frame); the merge loop with its lower_bound steps"""
    w1 = list(w1); w2 = list(w2)
    i = j = 0
    s = 0.0
    while i < len(w1) and j < len(w2):
        vi = float(v1[i]); wi = float(v2[j])
        if w1[i] == w2[j]:
            if scoring == L1_NORM:
                s += math.fabs(vi - wi) - math.fabs(vi) - math.fabs(wi)
            elif scoring in (L2_NORM, DOT_PRODUCT):
                s += vi * wi
            elif scoring == CHI_SQUARE:
                if vi + wi != 0.0:
                    s += vi * wi / (vi + wi)
            elif scoring == BHATTACHARYYA:
                s += math.sqrt(vi * wi)
            else:
                raise ValueError("KL is not restated")
            i += 1; j += 1
        elif w1[i] < w2[j]:
            i = bisect.bisect_left(w1, w2[j], i)
        else:
            j = bisect.bisect_left(w2, w1[i], j)
    if scoring == L1_NORM:
        s = -s / 2.0
    elif scoring == L2_NORM:
        s = 1.0 if s >= 1 else 1.0 - math.sqrt(1.0 - s)
    elif scoring == CHI_SQUARE:
        s = 2. * s
    return s


# ------------------------------------------------------------------------------------------------ the database
class KeyFrame:
    def __init__(self, slot, words, values):
        self.slot = slot; self.words = [int(w) for w in words]; self.values = [float(v) for v in values]
        self.neigh = []
        self.reloc_query = 0; self.reloc_words = 0; self.reloc_score = F32(0)      # KeyFrame.cc:36; the scores: defined as 0
        self.loop_query = 0; self.loop_words = 0; self.loop_score = F32(0)


class Database:
    def __init__(self, n_words, scoring=L1_NORM):
        self.n_words = n_words; self.scoring = scoring
        self.inverted = [[] for _ in range(n_words)]
        self.kf = {}
        self.query_id = 0                                        # the frame's / key frame's mnId: one per call, never 0

    def add(self, slot, words, values):
        assert slot not in self.kf
        k = KeyFrame(slot, words, values); self.kf[slot] = k
        for w in k.words:
            self.inverted[w].append(k)

    def erase(self, slot):
        k = self.kf.pop(slot, None)
        if k is None:
            return
        for w in k.words:
            lst = self.inverted[w]
            for i, e in enumerate(lst):
                if e is k:
                    del lst[i]
                    break

    def clear(self):
        self.inverted = [[] for _ in range(self.n_words)]
        self.kf = {}

    def set_covisible(self, slot, slots):
        self.kf[slot].neigh = [int(s) for s in slots]

    def n_slots(self):
        return max(self.kf) + 1 if self.kf else 0

    def kept(self, slot):
        k = self.kf[slot]
        return np.array([k.reloc_score, k.loop_score], np.float32)

    def _result(self, n_slots, order, sharing, max_common, min_common, n_scored, best_acc, scored, acc_match, mode, qid):
        words = np.zeros(n_slots, np.int32); sc = np.full(n_slots, np.nan, np.float32); acc = np.full(n_slots, np.nan, np.float32)
        best = np.full(n_slots, -1, np.int32)
        for k in self.kf.values():
            if (k.reloc_query if mode == RELOC else k.loop_query) == qid:
                words[k.slot] = k.reloc_words if mode == RELOC else k.loop_words
        for k, si in scored:
            sc[k.slot] = si
        for k, a, b in acc_match:
            acc[k.slot] = a; best[k.slot] = b.slot
        return dict(candidates=np.array([k.slot for k in order], np.int32), n_sharing=len(sharing), max_common=max_common, min_common=min_common,
                    n_scored=n_scored, best_acc_score=F32(best_acc), words=words, score=sc, acc=acc, best=best,
                    discovery=[k.slot for k in sharing])

    def query(self, words, values, mode=RELOC, min_score=0.0, connected=None):
        """DetectRelocalizationCandidates (mode RELOC) or DetectLoopCandidates (mode LOOP); n_slots is read before the call like the device's views"""
        words = [int(w) for w in words]; values = [float(v) for v in values]
        n_slots = self.n_slots()
        self.query_id += 1; qid = self.query_id
        min_score = F32(min_score)
        conn = set(int(c) for c in (connected if connected is not None and mode == LOOP else []))
        sharing = []
        for w in words:
            for k in self.inverted[w]:
                if mode == RELOC:
                    if k.reloc_query != qid:
                        k.reloc_words = 0; k.reloc_query = qid; sharing.append(k)
                    k.reloc_words += 1
                else:
                    if k.loop_query != qid:
                        k.loop_words = 0
                        if k.slot not in conn:
                            k.loop_query = qid; sharing.append(k)
                    k.loop_words += 1
        start = min_score if mode == LOOP else F32(0)
        if not sharing:
            return self._result(n_slots, [], sharing, 0, 0, 0, start, [], [], mode, qid)
        max_common = 0
        for k in sharing:
            n = k.reloc_words if mode == RELOC else k.loop_words
            if n > max_common:
                max_common = n
        min_common = int(F32(max_common) * F32(0.8))              # int minCommonWords = maxCommonWords*0.8f
        score_and_match = []; scored = []
        for k in sharing:
            if (k.reloc_words if mode == RELOC else k.loop_words) > min_common:
                si = F32(score(self.scoring, words, values, k.words, k.values))
                scored.append((k, si))
                if mode == RELOC:
                    k.reloc_score = si; score_and_match.append((si, k))
                else:
                    k.loop_score = si
                    if si >= min_score:
                        score_and_match.append((si, k))
        if not score_and_match:
            return self._result(n_slots, [], sharing, max_common, min_common, len(scored), start, scored, [], mode, qid)
        best_acc = start
        acc_match = []
        for si, k in score_and_match:
            best_score = si; acc = si; best_kf = k
            for nb in k.neigh[:10]:
                k2 = self.kf.get(nb)
                if k2 is None:
                    continue
                if mode == RELOC:
                    if k2.reloc_query != qid:
                        continue
                    s2 = k2.reloc_score
                else:
                    if not (k2.loop_query == qid and k2.loop_words > min_common):
                        continue
                    s2 = k2.loop_score
                acc = F32(acc + s2)
                if s2 > best_score:
                    best_kf = k2; best_score = s2
            acc_match.append((k, acc, best_kf))
            if acc > best_acc:
                best_acc = acc
        retain = F32(F32(0.75) * best_acc)
        out = []; seen = set()
        for k, acc, b in acc_match:
            if acc > retain and b.slot not in seen:
                out.append(b); seen.add(b.slot)
        return self._result(n_slots, out, sharing, max_common, min_common, len(scored), best_acc, scored, acc_match, mode, qid)


def run_script(db, script):
    """play a script on a database; the list of the queries' results"""
    out = []
    for op in script:
        if op[0] == "add":
            db.add(op[1], op[2], op[3])
        elif op[0] == "erase":
            db.erase(op[1])
        elif op[0] == "clear":
            db.clear()
        elif op[0] == "cov":
            db.set_covisible(op[1], op[2])
        elif op[0] == "query":
            out.append(db.query(op[1], op[2], op[3], op[4], op[5]))
        else:
            raise ValueError(op[0])
    return out


def Q(words, values, mode=RELOC, min_score=0.0, connected=None):
    return ("query", np.asarray(words, np.int32), np.asarray(values, np.float64), mode, min_score, connected)


def A(slot, words, values):
    return ("add", slot, np.asarray(words, np.int32), np.asarray(values, np.float64))


# ------------------------------------------------------------------------------------------------ random databases
def random_bag(rng, n_voc_words, n, norm="L1"):
    """n distinct words in ascending order with values > 0, normalised like the vocabulary's bags"""
    w = np.sort(rng.choice(n_voc_words, n, replace=False)).astype(np.int32)
    v = 0.05 + rng.rand(n)
    if norm == "L1":
        v = v / np.abs(v).sum()
    elif norm == "L2":
        v = v / math.sqrt((v * v).sum())
    return w, v.astype(np.float64)


def norm_of(scoring):
    return None if scoring == DOT_PRODUCT else ("L2" if scoring == L2_NORM else "L1")


def near_bag(rng, n_voc_words, base_w, n, keep, norm):
    """a bag of n words that shares about `keep` of them with base_w (a view of the same place)"""
    nk = min(int(round(keep * n)), len(base_w), n)
    a = rng.choice(base_w, nk, replace=False)
    rest = np.setdiff1d(np.arange(n_voc_words), a)
    b = rng.choice(rest, n - nk, replace=False)
    w = np.sort(np.concatenate([a, b])).astype(np.int32)
    v = 0.05 + rng.rand(n)
    if norm == "L1":
        v = v / v.sum()
    elif norm == "L2":
        v = v / math.sqrt((v * v).sum())
    return w, v


def random_script(seed, n_voc_words, slots, bag_sizes, scoring=L1_NORM, n_queries=2, query_size=None, mode=RELOC, holes=0, places=4):
    """a database at the given slot numbers: the key frames are views of `places` places (bags that share most of their words), so that
    several pass the min-common test and the covisible neighbours -- slots of the same place -- add up; `holes` of them are erased again.
    Then n_queries queries near a place, the loop ones with connected slots and a min_score of 0, inside the range of the scores, above them."""
    rng = np.random.RandomState(seed); norm = norm_of(scoring)
    slots = list(slots); script = []; bags = {}
    if not slots:
        w, v = random_bag(rng, n_voc_words, min(bag_sizes[0], n_voc_words), norm)
        return [Q(w, v, mode, 0.01 if mode == LOOP else 0.0, [] if mode == LOOP else None)]
    place_bags = [random_bag(rng, n_voc_words, min(max(bag_sizes), n_voc_words), norm)[0] for _ in range(places)]
    place_of = {}
    for i, s in enumerate(slots):
        n = min(bag_sizes[i % len(bag_sizes)], n_voc_words); p = i % places
        w, v = near_bag(rng, n_voc_words, place_bags[p], n, 0.85, norm)
        script.append(A(s, w, v)); place_of[s] = p; bags[s] = (w, v)
    live = list(slots)
    for s in rng.choice(slots, min(holes, len(slots)), replace=False).tolist():
        script.append(("erase", s)); live.remove(s)
    for s in live:
        same = [t for t in slots if place_of[t] == place_of[s] and t != s]       # erased ones may stay in a list: they are skipped
        nb = rng.choice(same, min(len(same), rng.randint(0, 11)), replace=False).tolist() if same else []
        if nb and rng.rand() < 0.2:
            nb[0] = int(rng.randint(0, 20000))                                  # an id out of range
        script.append(("cov", s, nb))
    qn = query_size or max(bag_sizes)
    for qi in range(n_queries):
        w, v = near_bag(rng, n_voc_words, place_bags[qi % places], min(qn, n_voc_words), 0.8, norm)
        if mode == LOOP:
            conn = rng.choice(live, min(len(live), 3), replace=False).tolist() if live else []
            sc = sorted(score(scoring, w, v, *bags[t]) for t in live if t not in conn)       # min_score: none, the upper quartile of all scores, above all
            script.append(Q(w, v, LOOP, [0.0, float(F32(sc[(3 * len(sc)) // 4])) if sc else 0.0, 4.0][qi % 3], conn))
        else:
            script.append(Q(w, v))
    return script


# ------------------------------------------------------------------------------------------------ crafted cases (L1 scoring on dyadic values:
# a common word adds min(query value, key-frame value) to the score, exactly)
N_CRAFT_WORDS = 125


def _bag(words, value):
    return np.asarray(words, np.int32), np.full(len(words), value, np.float64)


def case_best_differs():
    """slots 0 and 1 are each other's neighbours: both entries name slot 0 (the higher score) as pBestKF and collapse to one candidate; slot 2,
    alone, follows.  Slot 1 was added first, so it is discovered first and the kept candidate comes from ITS entry (pBestKF != pKFi)"""
    w = [3, 10, 11, 12, 13]
    return [A(1, *_bag(w, 0.0625)), A(0, *_bag(w, 0.125)), A(2, *_bag(w, 0.1875)), ("cov", 0, [1]), ("cov", 1, [0]), Q(*_bag(w, 0.25))]


def case_discovery_order():
    """slot order 2, 5, 9; discovery order 9 (it shares the query's word 1), then 5 and 2 by add order on word 4 -- and after slot 5 was erased
    and added again, 2 before 5"""
    q = _bag([1, 4, 7, 8], 0.25)
    base = [A(5, *_bag([4, 7, 8, 50], 0.25)), A(2, *_bag([4, 7, 8, 60], 0.25)), A(9, *_bag([1, 7, 8, 70], 0.25))]
    return base + [Q(*q), ("erase", 5), A(5, *_bag([4, 7, 8, 50], 0.25)), Q(*q)]


def case_min_common_boundary():
    """max_common 10 -> min_common 8: the slot with 8 common words is not scored, the one with 9 is"""
    q = _bag(range(20, 30), 0.0625)
    return [A(0, *_bag(range(20, 30), 0.0625)), A(1, *_bag(list(range(20, 29)) + [40], 0.0625)), A(2, *_bag(list(range(20, 28)) + [41, 42], 0.0625)), Q(*q)]


def case_stale_score(with_first_query=True):
    """query 2 scores slots 0 and 2; slot 1 shares one word with it (in the query, below min-common, not scored) and is slot 0's neighbour.
    What slot 0's entry adds is the score query 1 left on slot 1 -- or 0 when query 1 never ran"""
    q1 = _bag(range(50, 58), 0.125)
    q2 = _bag(range(10, 20), 0.0625)
    s = [A(0, *_bag(range(10, 20), 0.03125)), A(1, *_bag([10] + list(range(50, 57)), 0.125)), A(2, *_bag(range(10, 20), 0.025390625)), ("cov", 0, [1])]
    return s + ([Q(*q1)] if with_first_query else []) + [Q(*q2)]


def case_loop(with_connected=True, min_score=0.3):
    """slot 0 has the highest score and is connected to the query key frame: it is not discovered, not scored and no neighbour.  min_score
    0.3 keeps slot 3 (score 0.25) out of lScoreAndMatch although it is scored"""
    q = _bag(range(30, 38), 0.125)
    s = [A(0, *_bag(range(30, 38), 0.125)), A(1, *_bag(range(30, 38), 0.0625)), A(2, *_bag(range(30, 38), 0.046875)), A(3, *_bag(range(30, 38), 0.03125)),
         ("cov", 1, [0, 3]), ("cov", 2, [0])]
    return s + [Q(q[0], q[1], LOOP, min_score, [0] if with_connected else [])]


def case_strict_075():
    """acc 1.0, 0.75 and 0.75 + 2^-20: 0.75f * 1.0f is not exceeded by the second"""
    q = _bag([5, 6, 7, 8], 0.25)
    w2 = np.array([0.1875, 0.1875, 0.1875, 0.1875 + 2.0 ** -20])
    return [A(0, *_bag([5, 6, 7, 8], 0.25)), A(1, *_bag([5, 6, 7, 8], 0.1875)), ("add", 2, np.array([5, 6, 7, 8], np.int32), w2), Q(*q)]


CRAFTED = {
    "best_differs": case_best_differs, "discovery_order": case_discovery_order, "min_common_boundary": case_min_common_boundary,
    "stale_with": lambda: case_stale_score(True), "stale_without": lambda: case_stale_score(False),
    "loop_connected": lambda: case_loop(True), "loop_unconnected": lambda: case_loop(False), "loop_high_min_score": lambda: case_loop(True, 0.9),
    "strict_075": case_strict_075,
}
