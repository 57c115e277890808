"""The two GPU matrices cannot fall behind the code again, and the inputs of
the client-session tests can fail -- all on the CPU.

* Every declaration of include/*.h that takes a `first_fail` is a call of the
  verdict matrix (tests/verdict_cases.py MATRIX) or is left out with a reason.
* Every `__global__` kernel of amphora_amd/csrc/*.hip whose template head has
  `bool BIG` names, in tests/field_cases.py BIG_KERNELS, the test of
  tests/test_hip_primes.py that launches both of its forms, or is left out
  with a reason; the named tests exist and take the eight-prime fixture.
* FC.assert_session_coverage holds on every prime, party count and arrival
  order tests/test_hip_primes.py::test_client_session uses.
* A plain Python model of the session (accumulate party by party, then K_RV
  over the sums / K_MASK from the sums) agrees with the ``%`` references on
  FC.odo_rows, and with ONE planted error each it disagrees on every prime on
  which that error can matter: the rows are decisive.  In the style of
  tests/test_extent_harness.py.
"""
import glob
import os
import re

import pytest

from tests import field_cases as FC
from tests import verdict_cases as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the verdict matrix covers the headers ---------------------------------------------
def declarations_with_first_fail():
    """{function name: header} of every prototype with a `first_fail` parameter."""
    out = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "include", "*.h"))):
        src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
        for m in re.finditer(r"\b(amph_[a-z0-9_]+)\s*\(([^;{()]*)\)\s*;", src):
            if re.search(r"\bint64_t\s*\*\s*first_fail\b", m.group(2)):
                out[m.group(1)] = os.path.basename(path)
    return out


def test_the_verdict_matrix_covers_every_first_fail():
    found = declarations_with_first_fail()
    assert len(found) >= 22 and "amph_client_finish_mask_json_dev" in found and "amph_verify" in found
    assert not set(VC.MATRIX) & set(VC.MATRIX_LEFT_OUT)
    assert all(VC.MATRIX_LEFT_OUT.values())  # a written reason each
    known = set(VC.MATRIX) | set(VC.MATRIX_LEFT_OUT)
    for name, header in found.items():
        base = name[:-4] if name.endswith("_dev") else name
        assert name in known or base in known, "%s (%s) takes a first_fail and is in no verdict test" % (name, header)
    for name in known:  # no stale key
        assert name in found, "%s is not a declaration with a first_fail" % name
    # the _dev siblings run through their base names: the base is declared too
    for name in found:
        if name.endswith("_dev"):
            assert name[:-4] in found, name


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
def global_kernels():
    """{kernel: its template head or None} of every __global__ kernel."""
    out = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "amphora_amd", "csrc", "*.hip"))):
        src = open(path).read()
        for m in re.finditer(r"(?:template\s*<([^<>]*)>\s*)?__global__[^\n]*?\bvoid\s+(k_\w+)\s*\(", src):
            assert m.group(2) not in out, m.group(2)
            out[m.group(2)] = m.group(1)
    return out


def test_the_prime_matrix_covers_every_big_kernel():
    kernels = global_kernels()
    assert len(kernels) >= 50 and kernels["k_acc_b64"] and kernels["k_xdecs_init"] is None  # the regex finds both kinds
    big = {k for k, head in kernels.items() if head and re.search(r"\bbool\s+BIG\b", head)}
    assert {"k_rv", "k_acc_b64", "k_conv_json_seg", "k_open_post_seg"} <= big and "k_mask_sums" not in big
    assert not set(FC.BIG_KERNELS) & set(FC.BIG_KERNELS_LEFT_OUT)
    assert all(FC.BIG_KERNELS_LEFT_OUT.values())
    known = set(FC.BIG_KERNELS) | set(FC.BIG_KERNELS_LEFT_OUT)
    assert big - known == set(), "kernels with a BIG form that no test of test_hip_primes.py is named for"
    assert known - big == set(), "stale entries"
    src = open(os.path.join(ROOT, "tests", "test_hip_primes.py")).read()
    on_env = set(re.findall(r"^def (test_\w+)\(env\b", src, re.M))  # the fixture that is the eight primes
    for kernel, test in FC.BIG_KERNELS.items():
        assert test in on_env, "%s: %s is no test on the env fixture" % (kernel, test)
    big_primes = [pr.id for pr in FC.PRIMES if pr.big]
    assert big_primes == ["test", "max128", "min_big"] and len(FC.PRIMES) == 8  # both forms: three primes and five


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
