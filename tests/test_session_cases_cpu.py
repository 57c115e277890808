"""The two GPU matrices cannot fall behind the code again, and the inputs of
the client-session tests can fail -- all on the CPU.

* Every declaration of include/*.h that takes a `first_fail` or a per-object
  `first_fails` is a call of the verdict matrix (tests/verdict_cases.py MATRIX)
  or is left out with a reason; the parser is tested on prototypes of its own.
* Every `__global__` kernel of amphora_amd/csrc/*.hip that takes the field
  parameters (an `Fp` argument) names, in tests/field_cases.py BIG_KERNELS
  (template head with `bool BIG`) or FP_KERNELS (no BIG form), the test of
  tests/test_hip_primes.py that launches it on the eight primes, or is left
  out with a reason; a kernel with a `bool SEG` form names one test per form;
  the named tests exist and take the eight-prime fixture.
* Every tests/test_*.py has a row in tests/README.md.
* FC.assert_session_coverage holds on every prime, party count and arrival
  order tests/test_hip_primes.py::test_client_session uses.
* A plain Python model of the session (accumulate party by party, then K_RV
  over the sums / K_MASK from the sums) agrees with the ``%`` references on
  FC.odo_rows, and with ONE planted error each it disagrees on every prime on
  which that error can matter: the rows are decisive.  In the style of
  tests/test_extent_harness.py.
* The same for the K-secret session on the objects of VC.session_objects: a
  model that accumulates tile by tile into sums packed on the word table and
  gives one verdict per object equals the builder's references, and with ONE
  planted error each in the object lookup, the verdict index or the sums'
  address it changes a verdict or an output on both verdict primes at every
  party count: the layout is decisive.
"""
import functools
import glob
import os
import re
from collections import namedtuple

import pytest

from tests import field_cases as FC
from tests import verdict_cases as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the verdict matrix covers the headers ---------------------------------------------
FIRST_FAIL = r"first_fails?"


def prototypes_with(text, parameter):
    """The names, in order, of the prototypes in the header `text` that take an
    `int64_t*` whose name matches the pattern `parameter` (comments do not
    count).  tests/test_text_cases_cpu.py reads the text verdicts with it."""
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return [m.group(1) for m in re.finditer(r"\b(amph_[a-z0-9_]+)\s*\(([^;{()]*)\)\s*;", src)
            if re.search(r"\bint64_t\s*\*\s*(?:%s)\b" % parameter, m.group(2))]


def first_fail_prototypes(text):
    """... that take an `int64_t* first_fail` or an `int64_t* first_fails`."""
    return prototypes_with(text, FIRST_FAIL)


def declarations_with(parameter):
    """{function name: header} of every prototype of include/*.h with such a parameter."""
    out = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "include", "*.h"))):
        for name in prototypes_with(open(path).read(), parameter):
            out[name] = os.path.basename(path)
    return out


def declarations_with_first_fail():
    """{function name: header} of every prototype with a `first_fail(s)` parameter."""
    return declarations_with(FIRST_FAIL)


def test_the_parser_finds_both_spellings_and_nothing_else():
    text = """
    int amph_one(amph_ctx* ctx, const uint8_t* y, int64_t* first_fail);
    int amph_many(amph_s* s, uint8_t* out,
                  int64_t *first_fails, int64_t* bad_chars);
    /* int amph_commented(amph_ctx* ctx, int64_t* first_fail); */
    int amph_other(amph_ctx* ctx, int64_t* first_failure);
    int amph_none(amph_ctx* ctx, int64_t* bad_chars);
    """
    assert first_fail_prototypes(text) == ["amph_one", "amph_many"]


def check_verdict_matrix(found, matrix, left_out):
    assert not set(matrix) & set(left_out)
    assert all(left_out.values())  # a written reason each
    known = set(matrix) | set(left_out)
    for name, header in found.items():
        base = name[:-4] if name.endswith("_dev") else name
        assert name in known or base in known, "%s (%s) takes a first_fail and is in no verdict test" % (name, header)
    for name in known:  # no stale key
        assert name in found, "%s is not a declaration with a first_fail" % name
    # the _dev siblings run through their base names: the base is declared too
    for name in found:
        if name.endswith("_dev"):
            assert name[:-4] in found, name


def test_the_verdict_matrix_covers_every_first_fail():
    found = declarations_with_first_fail()
    assert len(found) >= 28 and "amph_client_finish_mask_json_dev" in found and "amph_verify" in found
    assert "amph_clients_finish_mask_json_dev" in found  # the per-object `first_fails` spelling
    check_verdict_matrix(found, VC.MATRIX, VC.MATRIX_LEFT_OUT)


def test_the_verdict_guard_misses_no_session_call():
    """Without its three K-secret entries the matrix is refused, by name."""
    short = {k: v for k, v in VC.MATRIX.items() if not k.startswith("amph_clients_")}
    assert len(short) == len(VC.MATRIX) - 3
    with pytest.raises(AssertionError, match=r"amph_clients_finish_verify \(amphora_client_batch.h\) takes a first_fail"):
        check_verdict_matrix(declarations_with_first_fail(), short, VC.MATRIX_LEFT_OUT)


def test_the_verdict_matrix_names_are_the_tests_parameters():
    """tests/test_hip_verdicts.py is a GPU module: its text is parsed, not imported."""
    src = open(os.path.join(ROOT, "tests", "test_hip_verdicts.py")).read()
    lists = {}
    for name in ("SINGLE_CALLS", "MANY_CALLS"):
        m = re.search(r"^%s = \[(.*?)\]" % name, src, re.S | re.M)
        lists[name] = re.findall(r'"(\w+)"', m.group(1))
    calls = lists["SINGLE_CALLS"] + lists["MANY_CALLS"]
    assert len(calls) == len(set(calls)) and set(calls) == set(VC.MATRIX.values())
    run = re.search(r"^RUN = \{(.*?)\}", src, re.S | re.M).group(1)
    assert set(re.findall(r'"(\w+)":', run)) == set(calls)


# ---- the prime matrix covers the kernels -------------------------------------------------
Kernel = namedtuple("Kernel", "head args")  # the template head (None without one), the argument list


def global_kernels():
    """{kernel: Kernel} of every __global__ kernel."""
    out = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "amphora_amd", "csrc", "*.hip"))):
        src = open(path).read()
        for m in re.finditer(r"(?:template\s*<([^<>]*)>\s*)?__global__[^\n]*?\bvoid\s+(k_\w+)\s*\(([^()]*)\)", src):
            assert m.group(2) not in out, m.group(2)
            out[m.group(2)] = Kernel(m.group(1), m.group(3))
        # (an argument list with a parenthesis in it would drop its kernel from the pattern above)
        assert set(re.findall(r"__global__[^\n]*?\bvoid\s+(k_\w+)\s*\(", src)) <= set(out), path
    return out


def has_flag(kernel, flag):
    return bool(kernel.head and re.search(r"\bbool\s+%s\b" % flag, kernel.head))


def test_the_prime_matrix_covers_every_big_kernel():
    """... and every kernel that takes the field parameters without a BIG form."""
    kernels = global_kernels()
    assert len(kernels) >= 50 and kernels["k_acc_b64"].head and kernels["k_xdecs_init"].head is None  # both kinds
    fp = {k for k, v in kernels.items() if re.search(r"\bFp\b", v.args)}  # takes the field parameters
    big = {k for k, v in kernels.items() if has_flag(v, "BIG")}
    seg = {k for k, v in kernels.items() if has_flag(v, "SEG")}
    assert {"k_rv", "k_acc_b64", "k_conv_json_seg", "k_open_post_seg"} <= big <= fp and seg == {"k_acc_b64"}
    assert {"k_mask_sums", "k_mask_sums_seg", "k_from_gfp", "k_odo_pre"} <= fp - big and "k_xdecs_init" not in fp
    tables = (FC.BIG_KERNELS, FC.BIG_KERNELS_LEFT_OUT, FC.FP_KERNELS, FC.FP_KERNELS_LEFT_OUT)
    assert sum(len(t) for t in tables) == len(set().union(*tables))  # a kernel stands in one table
    assert all(FC.BIG_KERNELS_LEFT_OUT.values()) and all(FC.FP_KERNELS_LEFT_OUT.values())
    known_big = set(FC.BIG_KERNELS) | set(FC.BIG_KERNELS_LEFT_OUT)
    known_fp = set(FC.FP_KERNELS) | set(FC.FP_KERNELS_LEFT_OUT)
    assert big - known_big == set(), "kernels with a BIG form that no test of test_hip_primes.py is named for"
    assert (fp - big) - known_fp == set(), "kernels that take Fp (no BIG form) that no test of test_hip_primes.py is named for"
    assert known_big - big == set() and known_fp - (fp - big) == set(), "stale entries"
    src = open(os.path.join(ROOT, "tests", "test_hip_primes.py")).read()
    on_env = set(re.findall(r"^def (test_\w+)\(env\b", src, re.M))  # the fixture that is the eight primes
    for kernel, tests in {**FC.BIG_KERNELS, **FC.FP_KERNELS}.items():
        if kernel in seg:  # one test per form: (SEG = false, SEG = true)
            assert isinstance(tests, tuple) and len(set(tests)) == 2, "%s: one test for each of its two forms" % kernel
        else:
            assert isinstance(tests, str), kernel
            tests = (tests,)
        for test in tests:
            assert test in on_env, "%s: %s is no test on the env fixture" % (kernel, test)
    assert FC.BIG_KERNELS["k_acc_b64"] == ("test_client_session", "test_clients_session")
    big_primes = [pr.id for pr in FC.PRIMES if pr.big]
    assert big_primes == ["test", "max128", "min_big"] and len(FC.PRIMES) == 8  # both forms: three primes and five


# ---- every test file is described ----------------------------------------------------------
def test_every_test_file_has_a_row_in_the_readme():
    files = {os.path.basename(p) for p in glob.glob(os.path.join(ROOT, "tests", "test_*.py"))}
    rows = re.findall(r"^\| `(test_\w+\.py)` \|", open(os.path.join(ROOT, "tests", "README.md")).read(), re.M)
    assert len(rows) == len(set(rows)), "a file with two rows"
    assert files - set(rows) == set(), "test files without a row in tests/README.md"
    assert set(rows) - files == set(), "rows of tests/README.md for files that are gone"


# ---- the predicates of a running sum -------------------------------------------------------
@pytest.mark.parametrize("pid", FC.PRIME_IDS)
def test_session_coverage_holds(pid):
    pr = FC.BY_ID[pid]
    for n in FC.PARTY_COUNTS:
        rows = FC.odo_rows(pid, n)
        orders = FC.session_orders(n)
        assert len(orders) == min(3, max(1, n)) and orders[0] == list(range(n))
        sums = [FC.running_sums(pr, rows, order) for order in orders]
        assert all(s == sums[0] for s in sums)  # a sum mod p: the same in any order
        assert [FC.from_gfp(pr, x) for x in sums[0][0]] == list(rows.ys)
        for order in orders:
            cov = FC.assert_session_coverage(pr, rows, order)
            if n >= 2:
                assert 0 <= cov["exact_p_at"] < rows.W
            assert (cov["carry_at"] is not None) == (pr.big and n >= 2)


def test_session_coverage_can_fail():
    """Rows without a word >= p, without a sum of p, and a claim of a carry
    below 2^127 are each refused."""
    pr = FC.BY_ID["m89"]
    rows = FC.odo_rows("m89", 2)
    canon = FC.Rows(rows.W, 2, tuple(tuple(tuple(w % pr.p for w in f) for f in o) for o in rows.odos), *rows[3:])
    with pytest.raises(AssertionError):
        FC.assert_session_coverage(pr, canon, [0, 1])
    flat = FC.Rows(4, 2, tuple(tuple((pr.p + 1,) * 4 for _ in range(5)) for _ in range(2)), *[(0,) * 4] * 5)
    cov = FC.session_coverage(pr, flat, [1, 0])
    assert (cov["exact_p"], cov["p_minus_1"], cov["carry"]) == (0, 0, 0) and cov["noncanon"] == [(4,) * 5] * 2
    with pytest.raises(AssertionError):
        FC.assert_session_coverage(pr, flat, [1, 0])
    big = FC.BY_ID["min_big"]
    zeros = FC.Rows(4, 2, tuple(tuple((big.p,) * 4 for _ in range(5)) for _ in range(2)), *[(0,) * 4] * 5)
    with pytest.raises(AssertionError):  # two parties on a BIG prime and no sum past 2^128
        FC.assert_session_coverage(big, zeros, [0, 1])


# ---- a Python model of the session, with one planted error each -----------------------------
BUGS = {
    # name: the primes on which it can matter
    "drop129": [pr.id for pr in FC.PRIMES if pr.big],  # below 2^127 a sum of canonical words is < 2^128
    "nocanon": FC.PRIME_IDS,  # every prime has words >= p below 2^128 (p itself)
    "gt": FC.PRIME_IDS,       # every prime has recombined zeros: a closing share lands the sum on p
    "mask_wrap": FC.PRIME_IDS,  # every prime has a secret below its mask
}


def model_add(p, a, b, bug):
    """mod_add: a 129-bit sum, one conditional subtract."""
    s = a + b
    hi = 0 if bug == "drop129" else s >> 128  # planted: the carry out of bit 127 is dropped
    s &= FC.MASK128
    ge = s > p if bug == "gt" else s >= p     # planted: a sum of exactly p stays p
    return (s - p) & FC.MASK128 if hi or ge else s


def model_canon(pr, x):
    """canon<BIG>: one conditional subtract (every word is < 2 p); else exact."""
    return (x - pr.p if x >= pr.p else x) if pr.big else x % pr.p


def model_mont(pr, a, b):
    return a * b * pow(FC.M128, -1, pr.p) % pr.p


def model_first_fail(pr, s):
    for i in range(len(s[0])):
        if model_mont(pr, s[0][i], s[1][i]) != s[3][i] or model_mont(pr, s[2][i], s[1][i]) != s[4][i]:
            return i
    return -1


def model_session(pr, rows, order, secrets, bug=None):
    """-> (the five sums, K_RV's verdict and secrets, K_MASK's verdict and words).
    Accumulate: sums start at 0, every party's word is canonicalised and added
    (planted `nocanon`: added raw).  K_RV takes the sums as one party's raw
    words (canon again); K_MASK trusts them: raw compares, and
    toGfp(secret) - sum with p added back on a borrow (planted `mask_wrap`: the
    difference wraps at 2^128 and is reduced once, as if the operands were any
    128-bit words)."""
    p = pr.p
    sums = []
    for k in range(5):
        col = [0] * rows.W
        for j in order:
            f = rows.odos[j][k]
            for i in range(rows.W):
                x = f[i] if bug == "nocanon" else model_canon(pr, f[i])
                col[i] = model_add(p, col[i], x, bug)
        sums.append(col)
    canon = [[model_canon(pr, x) for x in col] for col in sums]
    rv = (model_first_fail(pr, canon), [FC.from_gfp(pr, x) for x in canon[0]])
    masked = []
    for sec, y in zip(secrets, sums[0]):
        d = model_mont(pr, sec, pr.r2) - y
        if bug == "mask_wrap":
            d &= FC.MASK128
            d = d - p if d >= p else d
        elif d < 0:
            d += p
        masked.append(d)
    return sums, rv, (model_first_fail(pr, sums), masked)


def grid_secrets(pr, W):
    E = FC.edge_words(pr.p)
    return [E[(3 * i + i // len(E)) % len(E)] for i in range(W)]  # raw words, >= p included


@pytest.mark.parametrize("pid", FC.PRIME_IDS)
def test_the_rows_are_decisive(pid):
    pr = FC.BY_ID[pid]
    for n in (2, 3):
        rows = FC.odo_rows(pid, n)
        secrets = grid_secrets(pr, rows.W)
        assert any(FC.to_gfp(pr, s % pr.p) < FC.to_gfp(pr, y) for s, y in zip(secrets, rows.ys))  # a borrow in the mask
        for order in FC.session_orders(n):
            want = (FC.running_sums(pr, rows, order), (-1, list(rows.ys)),
                    (-1, FC.mask_words(pr, secrets, rows.ys)))
            assert model_session(pr, rows, order, secrets) == want, (n, order)
            for bug, primes in BUGS.items():
                got = model_session(pr, rows, order, secrets, bug)
                if pid in primes:
                    assert got != want, (bug, n, order)
                else:
                    assert got == want, (bug, n, order)  # cannot matter here: the model agrees


# ---- a Python model of the K-secret session, with one planted error each ---------------------
VERDICT_PRIMES = ["test", "m89"]  # tests/test_hip_verdicts.py PRIMES (held to it below)
SEG_BUGS = {
    "global_index": "first_fails[o] takes w0 + word, not word",
    "linear_tiles": "tiles cut the packed words every 192; a tile is charged to the object of its first word",
    "skip_empty": "the object lookup does not count empty objects: g(o) = woff[o] / 192 + (non-empty objects before o)",
    "last_wins": "an object's verdict is the last failing word seen, not the minimum",
    "sum_alias": "the accumulate adds at sums[word], not sums[w0 + word]",
}
# where each planted error shows on every (prime, party count): the layout makes it visible to the GPU test
SEG_CHANGES = {
    "global_index": {"verdict": True, "output": False},
    "linear_tiles": {"verdict": True, "output": True},   # words past the charged object's end are never added
    "skip_empty": {"verdict": False, "output": True},    # every real tile keeps its owner; no "[]" for an empty object
    "last_wins": {"verdict": True, "output": False},
    "sum_alias": {"verdict": True, "output": True},
}


def model_tiles(woff, bug=None):
    """-> ((object, first local word, end local word) of every workgroup with a
    real tile, the empty objects whose "[]" a workgroup writes).  A grid of
    T / 192 + K workgroups; workgroup w belongs to the LAST object o with
    g(o) = woff[o] / 192 + o <= w and owns its tile w - g(o), if the object has
    that many (wiretiles.hpp wire_tile_find / wire_tile_real)."""
    K, T, t = len(woff) - 1, woff[-1], VC.TILE
    size = [woff[o + 1] - woff[o] for o in range(K)]
    tiles, brackets = [], []
    if bug == "linear_tiles":
        for first in range(0, T, t):
            o = max(o for o in range(K) if woff[o] <= first < woff[o + 1])
            lo = first - woff[o]
            tiles.append((o, lo, min(lo + t, size[o])))  # (the kernel's own clamp: word < the object's words)
        return tuple(tiles), tuple(o for o in range(K) if size[o] == 0)
    g, rank = [], 0
    for o in range(K):
        g.append(woff[o] // t + (rank if bug == "skip_empty" else o))
        rank += size[o] > 0
    for w in range(T // t + K):
        o = max(o for o in range(K) if g[o] <= w)
        local = w - g[o]
        if local * t < size[o]:
            tiles.append((o, local * t, min(local * t + t, size[o])))
        elif size[o] == 0 and local == 0:
            brackets.append(o)
    return tuple(tiles), tuple(brackets)


@functools.lru_cache(maxsize=None)
def model_accumulate(pid, n, tiles, alias):
    """The five sums packed on the word table after every party is in: party by
    party, tile by tile, canon then add (planted `sum_alias`: at the object-local
    word).  Cached: three of the planted errors leave this step alone."""
    S = VC.session_objects(pid, n)
    pr = FC.BY_ID[pid]
    p, big = pr.p, pr.big
    sums = [[0] * S.woff[-1] for _ in range(5)]
    rows = [VC.object_rows(obj) for obj in S.objects]
    for j in FC.session_orders(n)[-1]:
        for o, lo, hi in tiles:
            w0 = 0 if alias else S.woff[o]
            for k in range(5):
                f, col = rows[o][j][k], sums[k]
                for i in range(lo, hi):
                    x = f[i]
                    if x >= p:  # canon<BIG>: one conditional subtract, else exact
                        x = x - p if big else x % p
                    s = col[w0 + i] + x
                    col[w0 + i] = s - p if s >= p else s
    return tuple(tuple(col) for col in sums)


def model_clients(S, bug=None):
    """-> (the sums, K_RV's (verdicts, secrets), K_MASK's (verdicts, masked
    words, framed texts)).  K_RV runs word-packed over the sums as one party's
    words (canon again), every word looking its object up; K_MASK runs tile by
    tile from the sums as they are.  One verdict per object, object-local and
    min-combined; a word no tile covered has no masked word (None), an empty
    object no workgroup visited no "[]"."""
    pr = FC.BY_ID[S.pid]
    p, woff, K, T = pr.p, S.woff, len(S.sizes), S.woff[-1]
    Ri = pow(FC.M128, -1, p)
    tiles, brackets = model_tiles(woff, bug)
    sums = model_accumulate(S.pid, S.n, tiles, bug == "sum_alias")

    def fails(s, g):
        return s[0][g] * s[1][g] * Ri % p != s[3][g] or s[2][g] * s[1][g] * Ri % p != s[4][g]

    def report(ff, o, local):
        v = woff[o] + local if bug == "global_index" else local
        if bug == "last_wins" or ff[o] < 0 or v < ff[o]:
            ff[o] = v

    canon = [[model_canon(pr, x) for x in col] for col in sums]
    rv_ff = [-1] * K
    for o in range(K):  # (seg_find: the object that holds packed word g)
        for g in range(woff[o], woff[o + 1]):
            if fails(canon, g):
                report(rv_ff, o, g - woff[o])
    secrets = [x * pr.rinv % p for x in canon[0]]
    packed_secrets = [x for obj in S.objects for x in obj.secrets]
    mk_ff, masked = [-1] * K, [None] * T
    for o, lo, hi in tiles:
        for i in range(lo, hi):
            g = woff[o] + i
            if fails(sums, g):
                report(mk_ff, o, i)
            d = packed_secrets[g] * pr.r2 * Ri % p - sums[0][g]
            masked[g] = d + p if d < 0 else d
    texts = []
    for o in range(K):
        words = masked[woff[o]:woff[o + 1]]
        if not words:
            texts.append(b"[]" if o in brackets else None)
        else:
            texts.append(None if None in words else VC.data_text(words))
    return [list(col) for col in sums], (rv_ff, secrets), (mk_ff, masked, texts)


def clients_reference(S):
    """The same triple from the builder's per-object references (``%`` on Python ints)."""
    pr = FC.BY_ID[S.pid]
    cols = [[x for obj in S.objects for x in obj.cols[k]] for k in range(5)]
    sums = [[FC.to_gfp(pr, x) for x in col] for col in cols]
    return (sums, (list(S.ff), [x for obj in S.objects for x in obj.y]),
            (list(S.ff), [x for obj in S.objects for x in obj.masked], [obj.text for obj in S.objects]))


def test_the_models_tiles_cover_every_word_once():
    S = VC.session_objects("m89", 3)
    tiles, brackets = model_tiles(S.woff)
    seen = [0] * S.woff[-1]
    for o, lo, hi in tiles:
        assert 0 <= lo < hi <= S.sizes[o] and lo % VC.TILE == 0 and hi - lo <= VC.TILE
        for i in range(lo, hi):
            seen[S.woff[o] + i] += 1
    assert seen == [1] * S.woff[-1]
    assert list(brackets) == [o for o, W in enumerate(S.sizes) if W == 0] and len(brackets) >= 4
    # (the two planted enumerations differ from it where they should: a tile that is cut short, a "[]" nobody writes)
    assert model_tiles(S.woff, "linear_tiles")[0] != tiles
    assert model_tiles(S.woff, "skip_empty") == (tiles, ())


def test_the_verdict_primes_are_the_gpu_matrix_s():
    src = open(os.path.join(ROOT, "tests", "test_hip_verdicts.py")).read()
    assert re.findall(r'"(\w+)"', re.search(r"^PRIMES = \[(.*?)\]", src, re.M).group(1)) == VERDICT_PRIMES
    assert [FC.BY_ID[pid].big for pid in VERDICT_PRIMES] == [True, False]


@pytest.mark.parametrize("n", FC.PARTY_COUNTS)
@pytest.mark.parametrize("pid", VERDICT_PRIMES)
def test_the_session_objects_are_decisive(pid, n):
    """VC.session_objects asserts its layout predicates when it is built; the
    unplanted model equals its references, and every planted error changes a
    verdict or an output (not the sums alone) on this prime and party count."""
    S = VC.session_objects(pid, n)
    want = clients_reference(S)
    got = model_clients(S)
    assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2]
    for bug, what in SEG_BUGS.items():
        got = model_clients(S, bug)
        assert got[1] != want[1] or got[2] != want[2], (bug, what)
        changed = {"verdict": got[1][0] != want[1][0] or got[2][0] != want[2][0],
                   "output": got[1][1] != want[1][1] or got[2][1:] != want[2][1:]}
        assert changed == SEG_CHANGES[bug], (bug, changed)
