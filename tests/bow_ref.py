"""Restatement of DBoW2's TemplatedVocabulary::transform (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1139-1271, BowVector.cpp:34-84,
FORB.cpp:81-101), of the text format (:1350-1436) and of ORBmatcher::SearchByBoW (src/ORBmatcher.cc:162-293) in numpy / pure Python, written
from reading them: Python floats are the reference's doubles, np.float32 its floats.  Also the generators of the vocabularies and the
crafted cases tests/test_bow.py checks on the CPU and tests/test_bow_gpu.py runs on the device."""
import math

import numpy as np

TF_IDF, TF, IDF, BINARY = 0, 1, 2, 3
L1_NORM, L2_NORM, CHI_SQUARE, KL, BHATTACHARYYA, DOT_PRODUCT = 0, 1, 2, 3, 4, 5
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def ham(a, b):
    return int(_POP[np.bitwise_xor(a, b)].sum())


def norm_of(scoring):
    """mustNormalize (ScoringObject.h:74-89): None, 'L1' or 'L2'"""
    return None if scoring == DOT_PRODUCT else ("L2" if scoring == L2_NORM else "L1")


# ------------------------------------------------------------------------------------------------ vocabularies
def make_vocabulary(k, L, seed, scoring=L1_NORM, weighting=TF_IDF, leaf_at_level1=False, dup_root=False, dup_leaf=False, zero_weight_every=0, weights=None):
    """a full k-ary tree of depth L with random node descriptors, rows subtree by subtree (not the breadth-first order the library renumbers
    to).  leaf_at_level1: the root's first child is a word (an unbalanced tree).  dup_root / dup_leaf:
    the second child of the root / of every last-level parent repeats the first child's descriptor (a tie the first must win).
    zero_weight_every: every such word has weight 0 (a stopped word).  weights: a function word index -> weight."""
    rng = np.random.RandomState(seed)
    parent, leaf, desc, weight = [], [], [], []

    def add(pid, level):
        nid = len(parent) + 1
        parent.append(pid); desc.append(rng.randint(0, 256, 32).astype(np.uint8))
        is_leaf = level == L or (leaf_at_level1 and level == 1 and pid == 0 and nid == 1)
        leaf.append(1 if is_leaf else 0); weight.append(0.0)
        return nid, is_leaf

    def grow(pid, level):
        kids = []
        for _ in range(k):                     # a node's k children first, then each child's subtree in turn: parents before children, which is
            kids.append(add(pid, level))       # all the format asks for, and neither breadth-first nor the library's own numbering
        if (dup_root and pid == 0) or (dup_leaf and level == L):
            desc[kids[1][0] - 1] = desc[kids[0][0] - 1].copy()
        for nid, is_leaf in kids:
            if not is_leaf:
                grow(nid, level + 1)

    grow(0, 1)
    w = 0
    for i in range(len(parent)):
        if leaf[i]:
            weight[i] = float(weights(w)) if weights else float(0.25 + rng.rand() * 8.0)
            if zero_weight_every and w % zero_weight_every == 0:
                weight[i] = 0.0
            w += 1
    return dict(k=k, L=L, scoring=scoring, weighting=weighting, parent=np.array(parent, np.int32), is_leaf=np.array(leaf, np.uint8),
                desc=np.array(desc, np.uint8).reshape(-1, 32), weight=np.array(weight, np.float64))


def empty_vocabulary(k=3, L=2):
    return dict(k=k, L=L, scoring=L1_NORM, weighting=TF_IDF, parent=np.zeros(0, np.int32), is_leaf=np.zeros(0, np.uint8), desc=np.zeros((0, 32), np.uint8),
                weight=np.zeros(0, np.float64))


def tree(voc):
    """children[id] in row order, is_leaf[id], word[id], level[id] (the root is node 0 at level 0)"""
    n = len(voc["parent"]) + 1
    children = [[] for _ in range(n)]; leaf = [False] * n; word = [-1] * n; level = [0] * n
    nw = 0
    for i, p in enumerate(voc["parent"]):
        nid = i + 1
        children[int(p)].append(nid); level[nid] = level[int(p)] + 1
        if voc["is_leaf"][i]:
            leaf[nid] = True; word[nid] = nw; nw += 1
    return children, leaf, word, level, nw


def write_text(voc, path):
    """the reference's text format: 'k L scoring weighting', then 'parent is_leaf b0 .. b31 weight' per node"""
    with open(path, "w") as f:
        f.write("%d %d %d %d\n" % (voc["k"], voc["L"], voc["scoring"], voc["weighting"]))
        for i in range(len(voc["parent"])):
            f.write("%d %d %s %s\n" % (voc["parent"][i], voc["is_leaf"][i], " ".join(str(int(b)) for b in voc["desc"][i]), repr(float(voc["weight"][i]))))


def descend(voc, T, d, levelsup):
    """transform(feature, word_id, weight, nid, levelsup): (word, weight, nid, short, had_tie).  short: the descent met a leaf above level
    L - levelsup, where the reference leaves nid uninitialised -- the defined behaviour is that leaf's id."""
    children, leaf, word, _, _ = T
    nid_level = voc["L"] - levelsup
    nid = 0 if nid_level <= 0 else None
    final, level, tie = 0, 0, False
    while True:
        level += 1
        nodes = children[final]
        final = nodes[0]; best = ham(d, voc["desc"][final - 1])
        for c in nodes[1:]:
            dd = ham(d, voc["desc"][c - 1])
            if dd < best:
                best, final = dd, c
            elif dd == best:
                tie = True
        if level == nid_level:
            nid = final
        if leaf[final]:
            break
    short = nid is None
    if short:
        nid = final
    return word[final], float(voc["weight"][final - 1]), nid, short, tie


def transform(voc, descs, levelsup):
    """transform(features, BowVector, FeatureVector, levelsup) as the arrays the library returns"""
    n = len(descs)
    out = dict(word_id=np.full(n, -1, np.int32), node_id=np.full(n, -1, np.int32), n_short=0)
    T = tree(voc)
    bow, fv = {}, {}
    if T[4] > 0:                                               # !empty()
        tf = voc["weighting"] in (TF_IDF, TF)
        for i in range(n):
            wid, w, nid, short, _ = descend(voc, T, descs[i], levelsup)
            if w > 0:
                out["word_id"][i] = wid; out["node_id"][i] = nid; out["n_short"] += int(short)
                if wid in bow:
                    if tf:
                        bow[wid] += w                           # addWeight; addIfNotExist keeps the first
                else:
                    bow[wid] = w
                fv.setdefault(nid, []).append(i)
        norm = norm_of(voc["scoring"])
        words = sorted(bow)
        if tf and bow and norm is None:
            nd = float(len(bow))
            for wd in words:
                bow[wd] /= nd
        if norm is not None:
            s = 0.0
            if norm == "L1":
                for wd in words:
                    s += math.fabs(bow[wd])
            else:
                for wd in words:
                    s += bow[wd] * bow[wd]
                s = math.sqrt(s)
            if s > 0.0:
                for wd in words:
                    bow[wd] /= s
    words = sorted(bow); nodes = sorted(fv)
    out["bow_word"] = np.array(words, np.int32); out["bow_value"] = np.array([bow[w] for w in words], np.float64)
    out["fv_node"] = np.array(nodes, np.int32)
    out["fv_start"] = np.cumsum([0] + [len(fv[x]) for x in nodes]).astype(np.int32)
    out["fv_index"] = np.array([i for x in nodes for i in fv[x]], np.int32)
    return out


# ------------------------------------------------------------------------------------------------ SearchByBoW
def three_maxima(counts):
    """ORBmatcher::ComputeThreeMaxima (src/ORBmatcher.cc:1630-1673)"""
    max1 = max2 = max3 = 0; ind1 = ind2 = ind3 = -1
    for i, s in enumerate(counts):
        if s > max1:
            max3, max2, max1 = max2, max1, s; ind3, ind2, ind1 = ind2, ind1, i
        elif s > max2:
            max3, max2 = max2, s; ind3, ind2 = ind2, i
        elif s > max3:
            max3 = s; ind3 = i
    if np.float32(max2) < np.float32(0.1) * np.float32(max1):
        ind2 = ind3 = -1
    elif np.float32(max3) < np.float32(0.1) * np.float32(max1):
        ind3 = -1
    return ind1, ind2, ind3


def rot_bin(a_kf, a_f, fold30=True):
    rot = np.float32(a_kf) - np.float32(a_f)
    if rot < 0.0:
        rot = np.float32(rot + np.float32(360.0))
    x = np.float32(rot * (np.float32(1.0) / np.float32(30)))
    b = int(math.floor(float(x) + 0.5))                        # round(): half away from zero, x >= 0
    return 0 if (b == 30 and fold30) else b


def search_by_bow(kf, fr, nnratio=0.7, check_orientation=True, th_low=50, ignore_claims=False, trace=None, fold30=True):
    """kf: dict(desc, node_id, has_map_point, angle); fr: dict(desc, node_id, angle).  Returns (match_kf per frame feature, n_matches).
    ignore_claims: the wrong parallel version (every key-frame feature sees all of the node's frame features; the last writer wins).
    trace: a list that receives (kf feature, best, second, best frame feature, accepted) per visited key-frame feature."""
    nF = len(fr["desc"]); match = np.full(nF, -1, np.int32)
    rows = lambda ids: {x: [i for i in range(len(ids)) if ids[i] == x] for x in sorted(set(int(v) for v in ids if v >= 0))}
    fk, ff = rows(kf["node_id"]), rows(fr["node_id"])
    hist = [[] for _ in range(30)]; nm = 0
    for node in sorted(fk):
        if node not in ff:
            continue
        for ik in fk[node]:
            if not kf["has_map_point"][ik]:
                continue
            b1, b2, bi = 256, 256, -1
            for i in ff[node]:
                if match[i] >= 0 and not ignore_claims:
                    continue
                d = ham(kf["desc"][ik], fr["desc"][i])
                if d < b1:
                    b2, b1, bi = b1, d, i
                elif d < b2:
                    b2 = d
            acc = b1 <= th_low and bool(np.float32(b1) < np.float32(nnratio) * np.float32(b2))
            if trace is not None:
                trace.append((ik, b1, b2, bi, acc))
            if acc:
                if match[bi] < 0:
                    nm += 1
                match[bi] = ik
                if check_orientation:
                    b = rot_bin(kf["angle"][ik], fr["angle"][bi], fold30)
                    if b < 30:                                  # (fold30=False: the wrong version that leaves bin 30 outside the histogram)
                        hist[b].append(bi)
    if check_orientation:
        keep = three_maxima([len(h) for h in hist])
        for b in range(30):
            if b in keep:
                continue
            for i in hist[b]:
                if match[i] >= 0:
                    match[i] = -1; nm -= 1
    return match, nm


# ------------------------------------------------------------------------------------------------ crafted cases
def flip(d, nbits, start=0):
    """d with bits start .. start + nbits - 1 flipped"""
    o = np.array(d, np.uint8).copy()
    for b in range(start, start + nbits):
        o[b >> 3] ^= np.uint8(1 << (b & 7))
    return o


def hand_vocabulary():
    """k = 2, L = 2: node 1 = 0x00.., node 2 = 0xFF..; words under node 1: node 3 = 0x00.. (word 0, weight 1), node 4 = 0x0F.. (word 1, weight 2);
    under node 2: node 5 = 0xFF.. (word 2, weight 4), node 6 = 0xF0.. (word 3, weight 0.5).  Rows: 1, 2, 3, 4, 5, 6."""
    d = lambda b: np.full(32, b, np.uint8)
    return dict(k=2, L=2, scoring=L1_NORM, weighting=TF_IDF, parent=np.array([0, 0, 1, 1, 2, 2], np.int32), is_leaf=np.array([0, 0, 1, 1, 1, 1], np.uint8),
                desc=np.stack([d(0), d(255), d(0), d(0x0F), d(255), d(0xF0)]), weight=np.array([0, 0, 1.0, 2.0, 4.0, 0.5]))


def hand_descriptors():
    """four descriptors: two in word 0, one in word 1, one in word 2"""
    z = np.zeros(32, np.uint8)
    return np.stack([flip(z, 3), flip(np.full(32, 0x0F, np.uint8), 5, 96), flip(z, 1, 200), flip(np.full(32, 255, np.uint8), 7, 8)])


def chain_case():
    """six frame features in one node, three key-frame features whose best is the same frame feature 0: key-frame feature 0 takes it, feature 1
    must fall back to its second choice (frame feature 2), feature 2 then finds both taken and takes its third (frame feature 4).  With claims
    ignored all three write frame feature 0."""
    rng = np.random.RandomState(77)
    base = rng.randint(0, 256, 32).astype(np.uint8)
    far = [np.bitwise_xor(base, rng.randint(0, 256, 32).astype(np.uint8)) for _ in range(3)]
    f = np.stack([flip(base, 2), far[0], flip(base, 12, 40), far[1], flip(base, 20, 90), far[2]])
    k = np.stack([flip(base, 1, 200), flip(base, 1, 210), flip(base, 1, 220)])
    kf = dict(desc=k, node_id=np.array([7, 7, 7], np.int32), has_map_point=np.ones(3, np.uint8), angle=np.zeros(3, np.float32))
    fr = dict(desc=f, node_id=np.full(6, 7, np.int32), angle=np.zeros(6, np.float32))
    return kf, fr


def pair_at(d_best, d_second, seed=5, n_extra=0):
    """one key-frame feature and a node of frame features at Hamming distances d_best (twice when d_second == d_best: a tie at positions 0 and 1)
    and d_second, then n_extra far ones"""
    rng = np.random.RandomState(seed)
    base = rng.randint(0, 256, 32).astype(np.uint8)
    fs = [flip(base, d_best, 0)]
    if d_second is not None:
        fs.append(flip(base, d_second, 256 - d_second) if d_second != d_best else flip(base, d_best, 100))
    for e in range(n_extra):
        fs.append(flip(base, 150 + e, 40))
    kf = dict(desc=base[None], node_id=np.array([3], np.int32), has_map_point=np.ones(1, np.uint8), angle=np.zeros(1, np.float32))
    fr = dict(desc=np.stack(fs), node_id=np.full(len(fs), 3, np.int32), angle=np.zeros(len(fs), np.float32))
    return kf, fr


def random_pair(n_kf, n_f, seed, n_nodes=12, noise=18, mp_rate=0.8):
    """frame features = noisy copies of a pool, key-frame features other noisy copies of the same pool, nodes by pool entry: many accepted
    matches, rejected ones and contested frame features; angles spread over the bins"""
    rng = np.random.RandomState(seed)
    pool = rng.randint(0, 256, (max(n_f // 2, 1), 32)).astype(np.uint8)

    def side(n):
        src = rng.randint(0, len(pool), n)
        d = pool[src].copy()
        for i in range(n):
            for b in rng.randint(0, 256, rng.randint(0, noise)):
                d[i, b >> 3] ^= np.uint8(1 << (b & 7))
        node = (src % n_nodes).astype(np.int32) * 3 + 1
        node[rng.rand(n) < 0.05] = -1
        return d, node, src

    kd, kn, ks = side(n_kf); fd, fn_, fs = side(n_f)
    base_angle = rng.rand(len(pool)).astype(np.float32) * 360
    ka = ((base_angle[ks] + np.where(rng.rand(n_kf) < 0.8, 45.0, rng.rand(n_kf) * 360)) % 360).astype(np.float32)
    kf = dict(desc=kd, node_id=kn, has_map_point=(rng.rand(n_kf) < mp_rate).astype(np.uint8), angle=ka)
    fr = dict(desc=fd, node_id=fn_, angle=base_angle[fs].astype(np.float32))
    return kf, fr


def big_node_case(seed=9):
    """one node with 130 frame features and 70 key-frame features: more than a wave of candidates, and claims in every chunk"""
    kf, fr = random_pair(70, 130, seed, n_nodes=1, noise=30, mp_rate=0.9)
    kf["node_id"][:] = 4; fr["node_id"][:] = 4
    fr["desc"][129] = flip(kf["desc"][0], 1); kf["has_map_point"][0] = 1     # a match in the third chunk of 64 candidates
    return kf, fr


def distinct_word_descriptors(voc, seed=12, tries=4000):
    """one descriptor per word: random descriptors, the first that lands in each word kept (a word's own descriptor need not descend to it: an
    ancestor's sibling may be nearer), so N features give N distinct words"""
    rng = np.random.RandomState(seed); T = tree(voc); seen = {}
    for _ in range(tries):
        d = rng.randint(0, 256, 32).astype(np.uint8)
        wid, w, _, _, _ = descend(voc, T, d, 0)
        if w > 0 and wid not in seen:
            seen[wid] = d
            if len(seen) == T[4]:
                break
    return np.stack([seen[k] for k in sorted(seen)][::-1])        # descending word order: the sort has work to do


def bin30_case():
    """21 features with an exact twin each, every pair in a node of its own (all accepted), the frame's angles 0 and the key frame's: 3 x 0
    (bin 0), 3 x 890 (890 / 30 = 29.67 rounds to bin 30, folded to 0; the matcher does not reduce angles), 5 x 60, 5 x 120, 5 x 180 (bins 2,
    4, 6).  Folded, bin 0 holds 6 and is the maximum: bins 0, 2, 4 stay and bin 6 goes, 16 matches.  Without the fold bin 0 holds 3 and
    bins 2, 4, 6 stay: only membership of bin 0 decides which features survive."""
    rng = np.random.RandomState(30)
    d = rng.randint(0, 256, (21, 32)).astype(np.uint8)
    ang = np.array([0] * 3 + [890] * 3 + [60] * 5 + [120] * 5 + [180] * 5, np.float32)
    node = np.arange(1, 22, dtype=np.int32)
    kf = dict(desc=d.copy(), node_id=node.copy(), has_map_point=np.ones(21, np.uint8), angle=ang)
    fr = dict(desc=d.copy(), node_id=node.copy(), angle=np.zeros(21, np.float32))
    return kf, fr


def tfidf_case():
    """(vocabulary, count): a weight whose repeated sum differs from weight * count in the last bit -- 0.1 six times is 0.6, 0.1 * 6 is
    0.6000000000000001"""
    return make_vocabulary(2, 1, 3, scoring=DOT_PRODUCT, weighting=TF_IDF, weights=lambda w: 0.1), 6
