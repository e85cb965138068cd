"""Inputs and expected values for tests/support/field_probe.hip (TEST INFRASTRUCTURE): the hand-written gfx950 field forms of
deep-prove_amd/csrc/gl64_gfx950.h and everything built from them, at their edges and on the inputs that take their rare paths.

The reference is Python integers and `%` (and the big-int Poseidon2 of l0_independent.py): nothing here comes from the product.

Input file: a sequence of blocks, each `[MAGIC, tag, mode, n, words_per_record]` followed by n records of u64 words. The probe runs one launch
per block, thread i on record i, so the ORDER of the records is the placement of the cases in the waves (64 consecutive records = one wave).
Output: one file of u64 words per section (a.bin .. e.bin), the blocks' outputs appended in input order; the parsers below know the layout.

Rare families (each makes the named block take its correction / set its deferred bit; p = 2^64 - 2^32 + 1, eps = 2^32 - 1):
  mul / mul_f     (s 2^48)(t 2^48), 1 <= s, t < 2^16: the product is s t 2^96, so hl = x1 = x0 = 0 and u = 0 < hh = s t: the high limb borrows;
                  2^i 2^j with 33 <= i <= 63, 96 <= i + j <= 126, j <= 63: the same with hh a power of two;
  fma             a = s 2^48, b = t 2^48, d < s t (7 2^48, 2^48 with d = 1 and 5 among them): u = d < hh;
  fma3_f          x = s 2^48, d = t 2^48 with all limbs 0, and (3 2^48, 5 2^48, A = 2);
  join3_f         B = 0x3FFFFF, C = (k << 20) | 0xFFFFF, 2 <= k <= 15, any A < 2^22: Hh.lo = 2^32 - 1, Hh.hi = k, so k eps + (Hh.lo : t.lo) carries.
"""
import functools

import numpy as np

from . import l0_independent as l0

P = (1 << 64) - (1 << 32) + 1
EPS = (1 << 32) - 1
M64 = (1 << 64) - 1
MAGIC = 0x4650524F42453031  # "FPROBE01"
SENTINEL = 0xD15EA5ED0BADC0DE
SMALL_K = (0, 1, 7, 1 << 31, (1 << 32) - 1)

TAG_FORM, TAG_CANON, TAG_LAZY, TAG_ACC, TAG_MADDW, TAG_LIN, TAG_PERM, TAG_PERM1 = 1, 2, 3, 5, 6, 7, 8, 9
A_OUT, B_OUT, CANON_OUT, LAZY_OUT, LIN_OUT, PERM_OUT, PERM1_OUT = 10, 3, 13, 6, 6, 44, 12
MAX_LAUNCH = (1 << 17) - 1

# the union of the edge lists of tests/support/field_check.cpp and tools/r04/mulbench2.hip
EDGES = sorted({0, 1, 2, 3, 6, 7, 8, EPS - 1, EPS, EPS + 1, EPS + 2, 1 << 33, 1 << 48, (1 << 48) + 1, (1 << 48) - 1, 1 << 61, 1 << 63, (1 << 63) + 1, (1 << 63) - 1,
                P - 2, P - 1, P, P + 1, P - EPS, P - EPS - 1, P - (1 << 32), P // 2, P // 2 + 1, M64, M64 - 1, M64 - EPS, M64 - EPS - 1,
                0xFFFFFFFE00000000, 0xFFFFFFFEFFFFFFFF, 0x00000001FFFFFFFF, 0xFFFFFFFF00000000, 0x1000000010000001})
ADDENDS = (0, 1, P - 1, M64, EPS, M64 - EPS)
assert {P, P + 1, M64, M64 - EPS, 1 << 48} <= set(EDGES)
KINDS = ("", "mul", "fma", "fma3", "join3")  # which block of a FORM record is on its rare path ("" = none by construction)


def _obj(a):
    return np.asarray(a, dtype=np.uint64).astype(object)


def _u64(rows):
    return np.array(rows, dtype=np.uint64)


class Block:
    def __init__(self, tag, mode, recs, **meta):
        self.tag, self.mode, self.recs, self.meta = tag, mode, np.ascontiguousarray(recs, dtype=np.uint64), meta
        assert self.recs.ndim == 2 and 0 < self.recs.shape[0] <= MAX_LAUNCH

    @property
    def n(self):
        return self.recs.shape[0]

    def words(self):
        return np.concatenate([np.array([MAGIC, self.tag, self.mode, self.n, self.recs.shape[1]], dtype=np.uint64), self.recs.ravel()])


# ------------------------------------------------------------------------------------------------ sections a and b: FORM records
# record = (a, b, d, x, e, A, B, C):  mul(a, b)  fma(a, b, d)  mul_small(a, k)  mul_f(a, b)  fma3_f(x, e, A, B, C)  join3_f(A, B, C);  e < p, limbs in their documented range
def _ordinary(rng, n):
    """canonical words and limb sums as the permutation makes them (at most 21 limbs of 22 / 22 / 20 bits): no rare path"""
    r = np.empty((n, 8), dtype=np.uint64)
    r[:, :5] = rng.integers(0, P, size=(n, 5), dtype=np.uint64)
    r[:, 5:7] = rng.integers(0, 21 << 22, size=(n, 2), dtype=np.uint64)
    r[:, 7] = rng.integers(0, 21 << 20, size=n, dtype=np.uint64)
    return r


def _with(base, **f):
    r = [int(v) for v in base]
    for k, v in f.items():
        r["abdxeABC".index(k)] = v
    return r


def _rare_families(rng):
    """{kind: records}; a record is ordinary in every block but the one its kind names"""
    fam = {k: [] for k in KINDS[1:]}
    base = iter(_ordinary(rng, 20000))
    for _ in range(10000):
        s, t = (int(v) for v in rng.integers(1, 1 << 16, size=2))
        fam["mul"].append(_with(next(base), a=s << 48, b=t << 48))
    for i in range(33, 64):
        for j in range(0, 64):
            if 96 <= i + j <= 126:
                fam["mul"].append(_with(next(base), a=1 << i, b=1 << j))
    for d in (1, 5):
        fam["fma"].append(_with(next(base), a=7 << 48, b=1 << 48, d=d))
    for _ in range(510):
        s, t = (int(v) for v in rng.integers(2, 1 << 16, size=2))
        fam["fma"].append(_with(next(base), a=s << 48, b=t << 48, d=int(rng.integers(0, min(s * t, 1 << 32)))))
    fam["fma3"].append(_with(next(base), x=3 << 48, e=5 << 48, A=2, B=0, C=0))
    for _ in range(1023):
        s, t = (int(v) for v in rng.integers(1, 1 << 16, size=2))
        fam["fma3"].append(_with(next(base), x=s << 48, e=t << 48, A=0, B=0, C=0))
    # (a join3 record is a fma3 operand too: its x e is an ordinary product, whose low words the limbs cannot push over)
    for k in range(2, 16):
        for A in [0, 1, (1 << 22) - 1] + [int(v) for v in rng.integers(0, 1 << 22, size=29)]:
            fam["join3"].append(_with(next(base), A=A, B=0x3FFFFF, C=(k << 20) | 0xFFFFF))
    return fam


def _bound_corners():
    """the documented bounds of fma3_f / join3_f: A, B in {0, 1, 2^22 - 1, 2^28 - 1}, C in {0, 1, 2^20 - 1, 2^24 - 1}, x any u64, d < p"""
    xs = (0, 1, EPS, EPS + 1, 1 << 48, (1 << 63) + 1, P - 1, P, P + 1, M64 - EPS, M64)
    ds = (0, 1, EPS, EPS + 1, 1 << 48, 1 << 63, P // 2, P - EPS, P - 2, P - 1)
    out = []
    for A in (0, 1, (1 << 22) - 1, (1 << 28) - 1):
        for B in (0, 1, (1 << 22) - 1, (1 << 28) - 1):
            for C in (0, 1, (1 << 20) - 1, (1 << 24) - 1):
                for x in xs:
                    for d in ds:
                        out.append([x, d, (A + B + C) & M64, x, d, A, B, C])
    assert len(out) == 7040
    return out


def _place(rare, ordinary, lanes):
    """one wave: `rare` records in the given lanes, ordinary ones elsewhere"""
    rare, ordinary = iter(rare), iter(ordinary)
    return [next(rare) if l in lanes else next(ordinary) for l in range(64)]


def form_blocks(seed=2024):
    rng = np.random.default_rng(seed)
    fam = _rare_families(rng)
    blocks = []
    # ---- launch 1: the edge grid, the bound corners, the families as whole waves, then the placements among ordinary lanes
    recs, kinds = [], []

    def put(rs, ks):
        recs.extend(rs); kinds.extend(ks)

    grid = []
    for a in EDGES:
        for b in EDGES:
            for d in ADDENDS:
                grid.append([a, b, d, b, a % P, d & ((1 << 28) - 1), (d >> 28) & ((1 << 28) - 1), (d >> 40) & ((1 << 24) - 1)])
    put(grid, [""] * len(grid))
    corners = _bound_corners()
    put(corners, [""] * len(corners))
    ordinary = iter(_ordinary(rng, 64 * 64).tolist())
    while len(recs) % 64:
        put([next(ordinary)], [""])
    for k in KINDS[1:]:  # whole waves of one family (the last one filled up with its first records)
        rs = fam[k] + fam[k][:(-len(fam[k])) % 64]
        put(rs, [k] * len(rs))
    for k in KINDS[1:]:
        pick = iter(fam[k][::max(1, len(fam[k]) // 160)] + fam[k][:160])
        for lanes in ({0}, {63}, {31, 32}, set(range(0, 64, 2)), set(range(1, 64, 2))):
            put(_place(pick, ordinary, lanes), [k if l in lanes else "" for l in range(64)])
    blocks.append(Block(TAG_FORM, 0, _u64(recs), kinds=kinds, canonical_random=False))
    # ---- 64 k + 1 threads: the single lane of the last wave is a rare case
    for k in KINDS[1:]:
        rs = [next(ordinary) for _ in range(128)] + [fam[k][1]]
        blocks.append(Block(TAG_FORM, 0, _u64(rs), kinds=[""] * 128 + [k], canonical_random=False))
    # ---- the call under `if (lane & 1)`: rare cases in the active and in the inactive half
    recs, kinds = [], []
    for k in KINDS[1:]:
        pick = iter(fam[k][3::max(1, len(fam[k]) // 200)] + fam[k][:200])
        for lanes in (set(range(64)), set(range(1, 64, 2)), set(range(0, 64, 2)), {0, 1}, {62, 63}):
            put(_place(pick, ordinary, lanes), [k if l in lanes else "" for l in range(64)])
    put([next(ordinary) for _ in range(63)] + [fam["mul"][7]], [""] * 63 + ["mul"])
    blocks.append(Block(TAG_FORM, 1, _u64(recs), kinds=kinds, canonical_random=False))
    # ---- 2^16 random any-u64 cases, 2^16 canonical ones
    n = 1 << 16
    r = np.empty((n, 8), dtype=np.uint64)
    r[:, :4] = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    r[:, 4] = rng.integers(0, P, size=n, dtype=np.uint64)
    r[:, 5:7] = rng.integers(0, 1 << 28, size=(n, 2), dtype=np.uint64)
    r[:, 7] = rng.integers(0, 1 << 24, size=n, dtype=np.uint64)
    blocks.append(Block(TAG_FORM, 0, r, kinds=[""] * n, canonical_random=False))
    blocks.append(Block(TAG_FORM, 0, _ordinary(rng, n), kinds=[""] * n, canonical_random=True))
    return blocks


def form_expected(block):
    """(n, 10) section a and (n, 3) section b values mod p, as object arrays of Python ints"""
    a, b, d, x, e, A, B, C = (_obj(block.recs[:, i]) for i in range(8))
    limbs = A + B * (1 << 22) + C * (1 << 44)
    ea = [a * b, a * b + d] + [a * k for k in SMALL_K] + [a * b, x * e + limbs, limbs]
    return np.stack([v % P for v in ea], axis=1), np.stack([(a * b) % P, (x * e + limbs) % P, limbs % P], axis=1)


def form_active(block):
    """lanes that run the call: all, or the odd ones under `if (lane & 1)`"""
    lane = np.arange(block.n) & 63
    return (lane & 1).astype(bool) if block.mode else np.ones(block.n, dtype=bool)


# ------------------------------------------------------------------------------------------------ section c
def wrapper_blocks(seed=77):
    rng = np.random.default_rng(seed)
    canon = [v for v in EDGES if v < P]
    rs = [[a, canon[(i + 2 * j + 1) % len(canon)], b, canon[(3 * i + j + 2) % len(canon)], canon[(i + j) % len(canon)], canon[(5 * i + 7 * j + 3) % len(canon)]]
          for i, a in enumerate(canon) for j, b in enumerate(canon)]
    rs += rng.integers(0, P, size=(4096, 6), dtype=np.uint64).tolist()
    blocks = [Block(TAG_CANON, 0, _u64(rs))]
    rs = [[a, EDGES[(i + 2 * j + 1) % len(EDGES)], b, EDGES[(3 * i + j + 2) % len(EDGES)], EDGES[(i + j) % len(EDGES)], EDGES[(5 * i + 7 * j + 3) % len(EDGES)]]
          for i, a in enumerate(EDGES) for j, b in enumerate(EDGES)]
    rs += rng.integers(0, 1 << 64, size=(4096, 6), dtype=np.uint64).tolist()
    blocks.append(Block(TAG_LAZY, 0, _u64(rs)))
    # ExAcc: `mode` rows (start, count, step, 0), then the pool as rows (c0, c1, 0, 0) of m extension values; value j of a record is pool[(start + j step) % m]
    pool = [[M64, M64], [M64, 0], [P, P - 1], [0, 0], [M64 - EPS, EPS]] + [[EDGES[i], EDGES[-1 - i]] for i in range(len(EDGES))] + rng.integers(0, 1 << 64, size=(86, 2), dtype=np.uint64).tolist()
    acc = [[start, count, step] for count in (1, 2, 3, 4096) for step in (0, 1, 5) for start in list(range(8)) + [len(pool) - 1, len(pool) - 3]]
    blocks.append(Block(TAG_ACC, len(acc), _u64([r + [0] for r in acc] + [p + [0, 0] for p in pool]), n_acc=len(acc), pool=pool))
    # mul_add_w(a, b, row sum of eight words): a and the words any u64, b < p (the internal diagonal)
    rs = [[M64, P - 1] + [M64] * 8, [M64, 0] + [M64] * 8, [0, P - 1] + [M64] * 8, [7 << 48, 1 << 48] + [1, 0, 0, 0, 0, 0, 0, 0], [P, P - 1] + [P] * 8, [M64 - EPS, P - EPS] + [M64 - EPS] * 8]
    w = rng.integers(0, 1 << 64, size=(2042, 10), dtype=np.uint64)
    w[:, 1] = rng.integers(0, P, size=2042, dtype=np.uint64)
    blocks.append(Block(TAG_MADDW, 0, _u64(rs + w.tolist())))
    return blocks


def wrapper_expected(block):
    """canonical expected words of one section-c block, (n, words) object array"""
    if block.tag == TAG_CANON:
        out = []
        for a0, a1, b0, b1, r0, r1 in block.recs.astype(object).tolist():
            a, b, r = (a0, a1), (b0, b1), (r0, r1)
            lerp = l0.ext_add(a, l0.ext_mul(r, l0.ext_sub(b, a)))
            lerp_base = l0.ext_add((a0, 0), l0.ext_mul(r, ((b0 - a0) % P, 0)))
            out.append([a0 * b0 % P, a0 * a0 % P, 7 * a0 % P, *l0.ext_mul(a, b), a0 * b0 % P, a1 * b0 % P, *lerp, *lerp_base, *l0.ext_inv(a)])
        return np.array(out, dtype=object)
    if block.tag == TAG_LAZY:
        out = []
        for a0, a1, b0, b1, r0, r1 in block.recs.astype(object).tolist():
            a, b, r = (a0, a1), (b0, b1), (r0, r1)
            out.append([*l0.ext_mul(a, b), *l0.ext_add(b, l0.ext_mul(r, a)), (b0 + r0 * a0) % P, r1 * a0 % P])
        return np.array(out, dtype=object)
    if block.tag == TAG_ACC:
        pool, out = block.meta["pool"], []
        for start, count, step, _ in block.recs[:block.meta["n_acc"]].astype(object).tolist():
            vs = [pool[(start + j * step) % len(pool)] for j in range(count)]
            out.append([sum(v[0] for v in vs) % P, sum(v[1] for v in vs) % P])
        return np.array(out, dtype=object)
    assert block.tag == TAG_MADDW
    r = block.recs.astype(object)
    return ((r[:, 0] * r[:, 1] + r[:, 2:].sum(axis=1)) % P).reshape(-1, 1)


def wrapper_out_words(block):
    return {TAG_CANON: block.n * CANON_OUT, TAG_LAZY: block.n * LAZY_OUT, TAG_MADDW: block.n}.get(block.tag) or 2 * block.meta["n_acc"]


# ------------------------------------------------------------------------------------------------ section d
def split3(x):
    return (x & 0x3FFFFF, (x >> 22) & 0x3FFFFF, x >> 44)


def lin_block(seed=5):
    """records (x, rc): lane i of a group of 8 holds word i and the round constant of its lane"""
    rng = np.random.default_rng(seed)
    groups = [[M64] * 8, [0] * 8, [P - 1] * 8]
    for hot in (1, M64, 1 << 22, 1 << 44, (1 << 22) - 1):
        groups += [[hot if i == j else 0 for i in range(8)] for j in range(8)]
    groups += rng.integers(0, 1 << 64, size=(21, 8), dtype=np.uint64).tolist()
    assert len(groups) % 8 == 0  # whole waves, the groups of a wave all different
    rcs = [0, M64] + l0.RC_EXT_INITIAL[0] + l0.RC_EXT_TERMINAL[3] + l0.RC_INTERNAL
    recs = [[int(x), rcs[(7 * g + i) % len(rcs)]] for g, grp in enumerate(groups) for i, x in enumerate(grp)]
    return Block(TAG_LIN, 0, _u64(recs))


def lin_expected(block):
    """(n, 6): the three limbs of circ(2 M4, M4) x + rc, then of the 8-lane sum, as the integer matrix applied limb by limb"""
    r = block.recs.astype(object).tolist()
    out = []
    for g in range(0, len(r), 8):
        limbs = [split3(x) for x, _ in r[g:g + 8]]
        for i in range(8):
            rc = split3(r[g + i][1])
            full = [sum(l0.M_E[i][j] * limbs[j][t] for j in range(8)) + rc[t] for t in range(3)]
            out.append(full + [sum(limbs[j][t] for j in range(8)) for t in range(3)])
    assert max(max(o) for o in out) < 1 << 32
    return np.array(out, dtype=object)


# ------------------------------------------------------------------------------------------------ section e
PERM_GROUPS = (1, 3, 8, 9)  # states per launch of one 64-lane block: a single group, some, a full wave, and a second trip with one group


@functools.lru_cache(maxsize=None)
def perm_states():
    rng = np.random.default_rng(99)
    states = [tuple(int(v) for v in rng.integers(0, P, size=8, dtype=np.uint64)) for _ in range(300)]
    return states + [(0,) * 8, (P - 1,) * 8, (0, 1, P - 1, 1 << 32, (1 << 32) - 1, P - (1 << 32), 2, 3)]


@functools.lru_cache(maxsize=None)
def perm_expected():
    """[(permutation of the state, compress(state[:4], state[4:]))] from the independent big-int permutation"""
    return [(l0.permute(list(s)), l0.compress(s[:4], s[4:])) for s in perm_states()]


def perm_blocks():
    """lane-parallel launches covering every state (the last launch wraps round to the first states), then one one-lane launch of all"""
    st, blocks, pos, gi = perm_states(), [], 0, 0
    while pos < len(st):
        g = PERM_GROUPS[gi % len(PERM_GROUPS)]
        idx = [(pos + j) % len(st) for j in range(g)]
        blocks.append(Block(TAG_PERM, 0, _u64([st[i] for i in idx]), idx=idx))
        pos += g; gi += 1
    blocks.append(Block(TAG_PERM1, 0, _u64(st), idx=list(range(len(st)))))
    return blocks


# ------------------------------------------------------------------------------------------------ the file
@functools.lru_cache(maxsize=None)
def plan():
    return {"form": form_blocks(), "wrap": wrapper_blocks(), "lin": [lin_block()], "perm": perm_blocks()}


def write_input(path):
    p = plan()
    np.concatenate([b.words() for sec in ("form", "wrap", "lin", "perm") for b in p[sec]]).tofile(path)
    return p


def read_words(path):
    return np.fromfile(path, dtype=np.uint64)
