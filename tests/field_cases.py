"""Edge primes, carry-chain operands and plain Python-int references shared by
tests/test_field_host.py, tests/test_oracle_primes.py,
tests/test_session_cases_cpu.py and tests/test_hip_primes.py.

Every reference here is written with ``%`` and ``pow`` on Python ints (no
Montgomery tricks); every coverage predicate is computed on the inputs alone,
never from the code under test.  An ordinary module, not a conftest.
"""
from __future__ import annotations

import functools
import random
from collections import namedtuple

import numpy as np

from oracle import amphora_oracle as O

M128 = 1 << 128
MASK128 = M128 - 1

Prime = namedtuple("Prime", "id p r rinv r2 big kmax")


def _prime(pid: str, p: int) -> Prime:
    r = M128 % p
    rinv = pow(r, -1, p) if p > 1 else 0
    return Prime(pid, p, r, rinv, r * r % p, p > (1 << 127), MASK128 // p)


# Primality of every entry was checked with Miller-Rabin when the table was
# written (tests/test_field_host.py::test_prime_table re-checks it).
PRIMES = [
    _prime("test", O.TEST_PRIME),        # control
    _prime("max128", 2 ** 128 - 159),    # largest 128-bit prime: 3p > 2^129, three 0xFFFFFFFF limbs
    _prime("min_big", 2 ** 127 + 29),    # smallest BIG prime: two zero limbs, 2p barely above 2^128
    _prime("m127", 2 ** 127 - 1),        # largest !BIG prime: n0 == 1, all-ones limbs
    _prime("m89", 2 ** 89 - 1),          # the small prime the suite already used in three places
    _prime("two_limb", 2 ** 64 - 59),    # p[2] = p[3] = 0
    _prime("one_limb", 2 ** 32 - 5),     # p[1..3] = 0
    _prime("three", 3),                  # the ABI's stated lower bound (R = 1)
]
PRIME_IDS = [pr.id for pr in PRIMES]
BY_ID = {pr.id: pr for pr in PRIMES}
PARTY_COUNTS = [1, 2, 3, 4, 5, 16]  # templated 1-4, the run-time form, AMPH_MAX_PARTIES

_rng = random.Random(0x5EED0001)
UNIFORM_WORDS = [_rng.getrandbits(128) for _ in range(8)]  # the eight fixed-seed uniform words
del _rng


def is_probable_prime(n: int) -> bool:
    if n < 2:
        return False
    for q in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        if n % q == 0:
            return n == q
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


@functools.lru_cache(maxsize=None)
def _edge_words(p: int) -> tuple:
    pr = _prime("", p)
    vals = {0, 1, 2, p - 2, p - 1, p, p + 1, (p - 1) // 2, (p + 1) // 2}
    for k in (2, pr.kmax):
        vals |= {k * p - 1, k * p, k * p + 1}
    vals |= {M128 - 1, M128 - p, 1 << 127}
    for x in (pr.r, pr.r2, pr.rinv):
        vals |= {x, p - x}
    for j in (1, 2, 3):
        vals |= {(1 << 32 * j) - 1, 1 << 32 * j, (1 << 32 * j) + 1}
    vals |= {0xFFFFFFFF << 32 * j for j in range(4)}
    alt = 0xFFFFFFFF00000000FFFFFFFF00000000
    vals |= {alt, alt ^ MASK128}
    vals |= set(UNIFORM_WORDS)
    return tuple(sorted(v for v in vals if 0 <= v < M128))


def edge_words(p: int) -> list:
    """The sorted edge set E of the prime, clipped to [0, 2^128)."""
    return list(_edge_words(p))


def canonical(words, p: int) -> list:
    return [w for w in words if w < p]


# ---- numpy <-> int ---------------------------------------------------------------
def arr(vals, width: int = 16) -> np.ndarray:
    """Ints as little-endian 16-byte words, reshaped to rows of `width` bytes."""
    b = b"".join(int(v).to_bytes(16, "little") for v in vals)
    return np.frombuffer(b, np.uint8).reshape(-1, width).copy()


def ints(a) -> list:
    raw = np.ascontiguousarray(a).tobytes()
    return [int.from_bytes(raw[i:i + 16], "little") for i in range(0, len(raw), 16)]


# ---- references on Python ints ---------------------------------------------------
def from_gfp(pr: Prime, word: int) -> int:
    return word * pr.rinv % pr.p


def to_gfp(pr: Prime, value: int) -> int:
    return value * pr.r % pr.p


def recombine(pr: Prime, party_words) -> list:
    """party_words: per party a list of raw words -> canonical secrets."""
    return [sum(from_gfp(pr, s[i]) for s in party_words) % pr.p for i in range(len(party_words[0]))]


def recombine_verify(pr: Prime, odos):
    """odos: per party (y, r, v, w, u) lists of raw words -> (secrets, first failing index or -1)."""
    cols = [recombine(pr, [o[k] for o in odos]) for k in range(5)]
    ys, rs, vs, ws, us = cols
    return ys, O.first_failing_index(pr.p, ys, rs, us, vs, ws)


def mask_words(pr: Prime, secrets, masks) -> list:
    """maskInput: raw secret (any 128-bit value), canonical mask -> wire word."""
    return [to_gfp(pr, (s - m) % pr.p) for s, m in zip(secrets, masks)]


def convert_share(pr: Prime, masked, tuples, key: int, use_zero: bool) -> list:
    """masked: raw words; tuples: (value, mac) raw words -> (value, mac) wire words
    (oracle.amphora_oracle.convert_to_secret_share, which states the operation)."""
    spdz = O.MpSpdzIntegrationUtils(pr.p, pr.r, pr.rinv)
    le = lambda x: int(x).to_bytes(16, "little")  # noqa: E731
    out = O.convert_to_secret_share(spdz, [le(m) for m in masked], str(key), [(le(a), le(b)) for a, b in tuples],
                                    use_zero)
    w = [int.from_bytes(out[i:i + 16], "little") for i in range(0, len(out), 16)]
    return list(zip(w[0::2], w[1::2]))


def signed_diff(pr: Prime, x_word: int, a_word: int) -> int:
    """multiplyShares: fromGfp(x) - fromGfp(a), signed, not reduced."""
    return from_gfp(pr, x_word) - from_gfp(pr, a_word)


def odo_pre(pr: Prime, ys, m1s, m2s, triples):
    """ys: W share words; m1s / m2s: W mask words each (r, v); triples: 2 W
    (a, b, c) words -> 2 W signed (d, e) pairs in FactorPair order."""
    out = []
    for i in range(len(ys)):
        t0, t1 = triples[2 * i], triples[2 * i + 1]
        out.append((signed_diff(pr, ys[i], t0[0]), signed_diff(pr, m1s[i], t0[1])))
        out.append((signed_diff(pr, m2s[i], t1[0]), signed_diff(pr, m1s[i], t1[1])))
    return out


def open_values(pr: Prime, party_signed) -> list:
    """recombineDiffs in canonical form: per value the parties' signed sum mod p."""
    return [sum(col) % pr.p for col in zip(*party_signed)]


def post_word(pr: Prime, D: int, E: int, triple, player0: bool) -> int:
    """multiplySharedSecrets + toGfp for one pair; D, E any integers."""
    a, b, c = (from_gfp(pr, t) for t in triple)
    z = c + D * b + E * a
    if player0:
        z += D * E
    return to_gfp(pr, z % pr.p)


def signed_arrays(signed_pairs=None, mags=None, negs=None):
    """(mag (P, 2, 16), neg (P, 2)) from signed ints, or from explicit
    magnitudes and sign flags (negative zero, magnitudes >= p)."""
    if signed_pairs is not None:
        mags = [(abs(a), abs(b)) for a, b in signed_pairs]
        negs = [(a < 0, b < 0) for a, b in signed_pairs]
    mag = arr([x for pr_ in mags for x in pr_]).reshape(-1, 2, 16)
    neg = np.array(negs, np.uint8).reshape(-1, 2)
    return mag, neg


def signed_of(mag, neg) -> list:
    m = ints(mag)
    g = np.asarray(neg).reshape(-1).tolist()
    v = [-x if s else x for x, s in zip(m, g)]
    return list(zip(v[0::2], v[1::2]))


# ---- coverage predicates (inputs only) -------------------------------------------
def dot2_pre_subtract(pr: Prime, x: int, y: int, u: int, v: int) -> int:
    """The value dot2_redc holds before its conditional subtracts:
    (x y + u v + m p) / 2^128 with m = -(x y + u v) p^-1 mod 2^128."""
    t = x * y + u * v
    m = (-t * pow(pr.p, -1, M128)) % M128
    assert (t + m * pr.p) % M128 == 0
    return (t + m * pr.p) >> 128


def post_dot2_operands(pr: Prime, D: int, E: int, triple, player0: bool):
    """What K_ODO_POST hands to dot2_redc for canonical opened D, E: player 0
    folds D E in as D ([b] + [E]), the others pass the raw b word."""
    a, b, _ = triple
    bb = (b % pr.p + to_gfp(pr, E)) % pr.p if player0 else b
    return D, bb, E, a


def dot2_coverage(pr: Prime, rows) -> dict:
    """rows: (x, y, u, v).  How many rows need 0 / 1 / 2 final subtracts, and
    how many have the second top-limb bit set (hi == 2)."""
    cov = {"sub0": 0, "sub1": 0, "sub2": 0, "hi1": 0, "hi2": 0}
    for x, y, u, v in rows:
        T = dot2_pre_subtract(pr, x, y, u, v)
        assert T < 3 * pr.p
        cov["sub%d" % (T // pr.p)] += 1
        if T >> 128:
            cov["hi%d" % (T >> 128)] += 1
    return cov


def assert_dot2_coverage(pr: Prime, rows):
    """0, 1 and 2 subtracts on every prime (T < 3p reaches [2p, 3p) with raw
    words near 2^128 whatever the prime); hi == 1 needs 3p > 2^128 and
    hi == 2 needs 3p > 2^129."""
    cov = dot2_coverage(pr, rows)
    assert cov["sub0"] and cov["sub1"] and cov["sub2"], (pr.id, cov)
    if 3 * pr.p > M128:             # hi >= 1 reachable: T < 3p can pass 2^128
        assert cov["hi1"] or cov["hi2"], (pr.id, cov)
    if 3 * pr.p > 2 * M128:          # hi == 2 only for p > 2/3 2^128 (of the table: max128)
        assert cov["hi2"], (pr.id, cov)
    else:
        assert cov["hi2"] == 0
    return cov


def sum_coverage(pr: Prime, pairs) -> int:
    """How many (a, b) canonical pairs sum past 2^128 (the 129th bit)."""
    return sum(1 for a, b in pairs if a + b >= M128)


def mont_product(pr: Prime, a: int, b: int) -> int:
    return a * b * pow(M128, -1, pr.p) % pr.p if pr.p > 1 else 0


def noncanonical_coverage(pr: Prime, words) -> dict:
    """Input words in [p, 2^128), and exact multiples of p among them."""
    nc = [w for w in words if w >= pr.p]
    return {"noncanon": len(nc), "multiples": sum(1 for w in nc if w % pr.p == 0)}


def assert_noncanonical(pr: Prime, words):
    cov = noncanonical_coverage(pr, words)
    assert cov["noncanon"] and cov["multiples"], (pr.id, cov)  # p < 2^128: p itself always fits


# ---- the rows every family slices ------------------------------------------------
def lift(pr: Prime, value: int, i: int) -> int:
    """A canonical value as the input word of index i: canonical on even
    words, + k p on odd ones where that fits (k = 1, or the largest that
    fits on every fourth word)."""
    if i % 2 == 0:
        return value
    k = (MASK128 - value) // pr.p
    if k == 0:
        return value
    return value + (k if i % 4 == 3 else 1) * pr.p


Rows = namedtuple("Rows", "W n odos ys rs vs ws us")


@functools.lru_cache(maxsize=None)
def odo_rows(pid: str, n: int) -> Rows:
    """Honest ODO rows for n parties on the grid: party 0's (y, r) words are
    exactly E x E, v and the other parties' shares walk E at other strides,
    and the last party's y and r cancel parties 1..n-2 so that the recombined
    (y, r) stay E x E mod p at every n (the products 0 and p - 1 stay
    reachable); w = y r and u = v r are computed with Python ints, the last
    party's w / u share closing the sum.  Closing shares are written canonical
    on even words and + k p on odd ones; at words 1 and 3 party 0's w / u
    share is chosen so that the closing share is 1 (1 + k p fits below 2^128
    on every prime: the closing party holds words >= p in all five fields)."""
    pr = BY_ID[pid]
    E = edge_words(pr.p)
    L = len(E)
    W = L * L
    parties = [[[0] * W for _ in range(5)] for _ in range(n)]
    for i in range(W):
        a, b = divmod(i, L)
        for j in range(n):
            if j == 0:
                y, r, v = E[a], E[b], E[(a + 3 * b + 1) % L]
            else:
                y, r, v = E[(a + j * b + j) % L], E[(b + 5 * j + a * j) % L], E[(7 * a + b + j) % L]
            parties[j][0][i], parties[j][1][i], parties[j][2][i] = y, r, v
        if n >= 2:  # the last party cancels parties 1..n-2: the (y, r) sums stay E x E (mod p)
            for k in (0, 1):
                others = sum(parties[j][k][i] for j in range(1, n - 1))
                parties[n - 1][k][i] = lift(pr, -others % pr.p, i + k)
    ys = recombine(pr, [o[0] for o in parties])
    rs = recombine(pr, [o[1] for o in parties])
    vs = recombine(pr, [o[2] for o in parties])
    ws = [y * r % pr.p for y, r in zip(ys, rs)]
    us = [v * r % pr.p for v, r in zip(vs, rs)]
    for k, col in ((3, ws), (4, us)):
        for i in range(W):
            rest = to_gfp(pr, col[i])
            for j in range(n - 1):
                sh = E[(i + 11 * j + k) % L]
                parties[j][k][i] = sh
                rest = (rest - sh) % pr.p
            if n >= 2 and i in (1, 3):  # the closing share is 1 here, so that + k p fits on every prime:
                # above 2^128 - 2^8 (max128) the walk alone leaves the closing party's w / u canonical
                parties[0][k][i] = (parties[0][k][i] + rest - 1) % pr.p
                rest = 1
            parties[n - 1][k][i] = lift(pr, rest, i)
    return Rows(W, n, tuple(tuple(tuple(f) for f in o) for o in parties), tuple(ys), tuple(rs), tuple(vs),
                tuple(ws), tuple(us))


def odo_arrays(rows: Rows, lo: int = 0, hi: int | None = None):
    """The rows as per-party 5-tuples of (W, 16) arrays (fresh copies)."""
    return [tuple(arr(f[lo:hi]) for f in o) for o in rows.odos]


def fault_positions(W: int):
    return [0, W - 1, W // 2]


def with_fault(odos, index: int):
    """Copies of the arrays with party 0's w word at `index` off by one.
    Faults in y, r, v and u, by other parties, and changes that are no fault
    mod p are catalogued in tests/verdict_cases.py."""
    out = [tuple(f.copy() for f in o) for o in odos]
    w = out[0][3]
    v = int.from_bytes(w[index].tobytes(), "little")
    v = v + 1 if v < MASK128 else v - 1  # off by one without wrapping (2^128 - 1 -> 0 is no fault mod 3)
    w[index] = np.frombuffer(v.to_bytes(16, "little"), np.uint8)
    return out


def rv_coverage(pr: Prime, rows: Rows):
    """K_RV's predicates on the rows: a Montgomery product (the kernel's
    [y][r] R^-1 on the canonical sums) equal to 0 and to p - 1, input words
    >= p and multiples of p in every field, and at n >= 2 on a BIG prime a
    party sum that needs the 129th bit."""
    Rinv = pow(M128, -1, pr.p)
    sums = [[sum(o[k][i] % pr.p for o in rows.odos) % pr.p for i in range(rows.W)] for k in range(2)]
    prods = {a * b * Rinv % pr.p for a, b in zip(*sums)}
    assert 0 in prods and pr.p - 1 in prods, pr.id
    for k in range(5):
        assert_noncanonical(pr, [w for o in rows.odos for w in o[k]])
    if pr.big and rows.n >= 2:
        carries = 0
        for k in range(5):
            for i in range(rows.W):
                acc = rows.odos[0][k][i] % pr.p
                for o in rows.odos[1:]:
                    x = o[k][i] % pr.p
                    carries += acc + x >= M128
                    acc = (acc + x) % pr.p
        assert carries, pr.id


# ---- a running sum: the client session takes the parties one at a time -------------
def session_orders(n: int) -> list:
    """The arrival orders the session tests use: forward, reverse and one
    fixed permutation (odd slots first, then the even ones); equal orders
    (n <= 2) once."""
    fwd = list(range(n))
    out = []
    for order in (fwd, fwd[::-1], fwd[1::2] + fwd[0::2]):
        if order not in out:
            out.append(order)
    return out


def session_coverage(pr: Prime, rows: Rows, order) -> dict:
    """What a running sum per field meets when the parties of `rows` arrive in
    `order`: acc starts at 0 and every step adds the party's canonical word,
    acc = (acc + x mod p) mod p.  Counted over all five fields:

    * carry      steps with acc + x >= 2^128 (the add needs its 129th bit);
    * exact_p    steps with acc + x == p (the final subtract's equality);
    * p_minus_1  steps with acc + x == p - 1 (the largest sum left alone);
    * noncanon   per party (by slot) its five per-field counts of words >= p;

    with a witness each for the tests that read single words back: carry_at /
    exact_p_at, the smallest word index with such a step, an inner word
    (neither 0 nor W - 1) where there is one (None if no step qualifies).
    Python ints on the inputs alone."""
    p = pr.p
    cov = {"carry": 0, "exact_p": 0, "p_minus_1": 0,
           "noncanon": [tuple(sum(1 for w in f if w >= p) for f in o) for o in rows.odos]}
    at = {"carry": set(), "exact_p": set()}
    for k in range(5):
        fields = [rows.odos[j][k] for j in order]
        for i in range(rows.W):
            acc = 0
            for f in fields:
                s = acc + f[i] % p
                if s >= M128:
                    cov["carry"] += 1
                    at["carry"].add(i)
                if s == p:
                    cov["exact_p"] += 1
                    at["exact_p"].add(i)
                elif s == p - 1:
                    cov["p_minus_1"] += 1
                acc = s - p if s >= p else s
    for name, seen in at.items():
        inner = [i for i in seen if 0 < i < rows.W - 1]
        cov[name + "_at"] = min(inner or seen, default=None)
    return cov


def assert_session_coverage(pr: Prime, rows: Rows, order) -> dict:
    """Sums of exactly p and p - 1 at n >= 2 on every prime; a carry out of bit
    127 at n >= 2 on a BIG prime and never otherwise (2 p <= 2^128 below
    2^127, and the first party is added to 0); words >= p in every field of
    the party that arrives first and of the one that arrives last."""
    assert sorted(order) == list(range(rows.n)), order
    cov = session_coverage(pr, rows, order)
    if rows.n >= 2:
        assert cov["exact_p"] and cov["p_minus_1"], (pr.id, rows.n, order, cov)
    if pr.big and rows.n >= 2:
        assert cov["carry"] and cov["carry_at"] is not None, (pr.id, rows.n, order, cov)
    else:
        assert cov["carry"] == 0, (pr.id, rows.n, order, cov)
    for j in (order[0], order[-1]):
        assert all(cov["noncanon"][j]), (pr.id, rows.n, j, cov["noncanon"][j])
    return cov


def running_sums(pr: Prime, rows: Rows, order) -> list:
    """The five canonical Montgomery sums after every party of `order` is in:
    [k][i], the word the session holds for field k of word i
    (amph_client_word returns from_gfp of it)."""
    return [[sum(rows.odos[j][k][i] % pr.p for j in order) % pr.p for i in range(rows.W)] for k in range(5)]


# ---- which test launches both forms of a `template <..., bool BIG, ...>` kernel --------
# {kernel: the test of tests/test_hip_primes.py that runs it on all eight primes (three BIG, five not)};
# tests/test_session_cases_cpu.py holds this table against amphora_amd/csrc/*.hip.
BIG_KERNELS = {
    "k_rv": "test_recombine_verify",
    "k_mask": "test_mask_input",
    "k_rv_seg": "test_packed",
    "k_mask_seg": "test_packed",
    "k_recombine": "test_recombine_then_verify_columns",
    "k_verify": "test_recombine_then_verify_columns",
    "k_conv": "test_convert_share",
    "k_conv_json": "test_convert_share",
    "k_conv_json_seg": "test_convert_share_json_packed",
    "k_open": "test_open_and_post",
    "k_odo_post": "test_open_and_post",
    "k_open_post": "test_open_and_post",
    "k_open_post_seg": "test_party_sessions",
    "k_to_gfp": "test_codecs",
    "k_mask_words": "test_codecs",
    "k_synth": "test_device_synth",
    "k_synth_words": "test_device_synth",
    "k_rv_b64": "test_wire_fused",
    "k_mask_b64": "test_wire_fused",
    "k_mask_json": "test_wire_fused",
    "k_rv_b64_seg": "test_wire_packed",
    "k_mask_b64_seg": "test_wire_packed",
    "k_mask_json_seg": "test_wire_packed",
    # `bool SEG` besides `bool BIG`: one test per form, (SEG = false: one secret, SEG = true: K secrets)
    "k_acc_b64": ("test_client_session", "test_clients_session"),
}
BIG_KERNELS_LEFT_OUT = {}  # {kernel: why no test of test_hip_primes.py launches both of its forms}

# Kernels that take the field parameters (an `Fp` argument) and have no BIG form: one code path
# for every prime, so the guard that keys on `bool BIG` cannot see them.  {kernel: the test of
# tests/test_hip_primes.py whose calls reach its launcher on all eight primes}.
FP_KERNELS = {
    "k_mask_sums": "test_client_session",       # amph_client_finish_mask / _mask_json -> launch_mask_sums
    "k_mask_sums_seg": "test_clients_session",  # amph_clients_finish_mask / _mask_json -> launch_mask_sums_seg
    "k_from_gfp": "test_codecs",                # amph_from_gfp -> launch_from_gfp
    "k_odo_pre": "test_odo_pre",                # amph_odo_pre -> launch_odo_pre
}
FP_KERNELS_LEFT_OUT = {}  # {kernel: why no test of test_hip_primes.py launches it}


PostRows = namedtuple("PostRows", "W triples own partners")


@functools.lru_cache(maxsize=None)
def post_rows(pid: str, n: int) -> PostRows:
    """Beaver rows: 2 W pairs with triples (a, b, c) from the grid, this
    party's own signed diffs as K_ODO_PRE derives them from share / mask words
    of the grid, and n - 1 partners' (magnitude, negative) lists.  The first
    named pairs are steered to the dot2_redc corners: D = E = p - 1 against
    a = b = 2^128 - 1 (hi == 2 on max128, two subtracts everywhere), D = E = 0,
    D = E = 1.  At n >= 2 all six are steered through partner 1's magnitudes;
    at n = 1 the even ones (0, 2, 4: a word's two pairs share its mask word)
    through this party's own share and mask words.
    Partner magnitudes come from E raw -- 0 and p with the negative flag, >= p,
    2^128 - 1 -- with both signs."""
    pr = BY_ID[pid]
    E = edge_words(pr.p)
    L = len(E)
    P2 = L * L // 2 * 2  # pairs (even: 2 per word)
    W = P2 // 2
    top = MASK128
    named = [((pr.p - 1, pr.p - 1), (top, top, top)), ((0, 0), (top, top, 0)), ((1, 1), (top - 1, top, 1)),
             ((pr.p - 1, 1), (pr.p, top, pr.p - 1)), ((pr.p - 1, pr.p - 1), (pr.p - 1, pr.p - 1, pr.p - 1)),
             ((pr.p // 2, pr.p - 1), (top, 1 << 127, 0))]
    triples, ys, m1s, m2s = [], [], [], []
    for k in range(P2):
        i, j = divmod(k, L)
        if k < len(named):
            triples.append(named[k][1])
        else:
            triples.append((E[i % L], E[j], E[(i + 2 * j + 1) % L]))
    for w in range(W):
        ys.append(E[(5 * w + 1) % L])
        m1s.append(E[(w // L + 3 * w) % L])
        m2s.append(E[(7 * w + 2) % L])
    if n == 1:  # no partner to steer through: the even named pairs get the share / mask words that open to the target
        for k in range(0, len(named), 2):
            (D, Ev), (a, b, _) = named[k]
            ys[k // 2] = lift(pr, to_gfp(pr, (D + from_gfp(pr, a)) % pr.p), k // 2)
            m1s[k // 2] = lift(pr, to_gfp(pr, (Ev + from_gfp(pr, b)) % pr.p), k // 2 + 1)
    own = odo_pre(pr, ys, m1s, m2s, triples)
    partners = []
    for q in range(1, n):
        mags, negs = [], []
        for k in range(P2):
            i, j = divmod(k, L)
            mags.append((E[(i + q) % L], E[(j + 3 * q) % L]))
            negs.append(((k + q) % 2, (k // 2 + i + q) % 2))
        partners.append((mags, negs))
    if n >= 2:  # steer the named pairs through partner 1
        mags, negs = partners[0]
        for k, (target, _) in enumerate(named):
            others = [tuple((-m if g else m) for m, g in zip(pm[k], pg[k])) for pm, pg in partners[1:]]
            need = []
            for c in range(2):
                have = own[k][c] + sum(o[c] for o in others)
                need.append((target[c] - have) % pr.p)
            # as a negative magnitude on odd named pairs: -(p - need) == need (mod p)
            if k % 2:
                mags[k] = tuple((pr.p - x) % pr.p for x in need)
                negs[k] = (1, 1)
            else:
                mags[k] = tuple(need)
                negs[k] = (0, 0)
        # negative zero, negative p and 2^128 - 1 with both signs, whatever the walk gave
        base = len(named)
        for off, (m, g) in enumerate([((0, 0), (1, 1)), ((pr.p, pr.p), (1, 1)), ((top, top), (0, 1)),
                                      ((top, 0), (1, 0)), ((pr.p, 0), (0, 1))]):
            mags[base + off], negs[base + off] = m, g
    return PostRows(W, tuple(triples), (tuple(ys), tuple(m1s), tuple(m2s), tuple(own)),
                    tuple((tuple(m), tuple(g)) for m, g in partners))


def post_party_signed(rows: PostRows):
    """Every party's signed (d, e) list: own first, then the partners."""
    out = [list(rows.own[3])]
    for mags, negs in rows.partners:
        out.append([tuple((-m if g else m) for m, g in zip(pm, pg)) for pm, pg in zip(mags, negs)])
    return out


def post_opened(pr: Prime, rows: PostRows):
    signed = post_party_signed(rows)
    flat = [[x for pair in party for x in pair] for party in signed]
    o = open_values(pr, flat)
    return list(zip(o[0::2], o[1::2]))


def post_expected(pr: Prime, rows: PostRows, opened, player0: bool):
    z = [post_word(pr, D, E, t, player0) for (D, E), t in zip(opened, rows.triples)]
    return z[0::2], z[1::2]


def post_dot2_rows(pr: Prime, rows: PostRows, opened, player0: bool):
    return [post_dot2_operands(pr, D, E, t, player0) for (D, E), t in zip(opened, rows.triples)]
