"""amphora_amd/csrc/field.hpp on the host against Python ints: every function
of the header over the edge grid E x E of every prime in
tests/field_cases.py, bit-exact, through the stand-alone driver
tests/cpp/field_test.cpp (plain build, and the same program under
ASan + UBSan).  This pins the algorithms (CIOS and product-scanning Montgomery
products, redc, dot2_redc's two-bit top limb, the 129-bit add) and the host
fallbacks of addc / subc / macc96; the device builtins and the inline assembly
are pinned on the GPU by tests/test_hip_primes.py.  CPU only.

Operands respect each function's contract (field.hpp): mont_mul a < 2^128,
b < p; redc a < 2^128; dot2_redc x, u < p and y, v < 2^128; mod_add / mod_sub
a, b < p; canon<true> only for p > 2^127.

What these vectors tell apart (tried on copies of the header): dot2_redc with
one final subtract instead of two fails on every prime; its `hi >= b` test
replaced by `b == 0` fails on the four primes with 3p > 2^128 (hi is 0
below); reduce_once ignoring hi fails on the three BIG primes (mod_add, and
on 2^128 - 159 both Montgomery products).  redc's t4 carry cannot be told
from zero by any input: with V_-1 = a < 2^128 and V_i = (V_i-1 + m_i p) / 2^32
<= (2^128 - 1 + (2^32 - 1) p) / 2^32 < 2^128 for p < 2^128, no step of redc
ever carries into t4.
"""
import os
import subprocess
import sys

import pytest

from tests import field_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def binary(request):
    import build_native
    return build_native.build_field_test(sanitize=request.param == "sanitized")


def run_lines(binary, lines):
    text = "\n".join(lines) + "\n"
    r = subprocess.run([binary], input=text, capture_output=True, text=True, timeout=300, env=_ENV)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
    got = [int(x, 16) for x in r.stdout.split()]
    assert len(got) == len(lines)
    return got


def dot2_rows(pr):
    """(x, y, u, v): (x, y) over Ecanon x E with (u, v) walking the grid at
    other strides, the mirrored and the one-product rows, and the named
    corners (p - 1, 2^128 - 1 twice: the largest sum)."""
    E = FC.edge_words(pr.p)
    Ec = FC.canonical(E, pr.p)
    rows = [(pr.p - 1, FC.MASK128, pr.p - 1, FC.MASK128), (0, 0, 0, 0), (pr.p - 1, pr.p - 1, pr.p - 1, pr.p - 1)]
    for i, x in enumerate(Ec):
        for j, y in enumerate(E):
            rows.append((x, y, Ec[(7 * i + 3 * j + 1) % len(Ec)], E[(5 * i + 11 * j + 2) % len(E)]))
            rows.append((x, y, x, y))
            rows.append((x, y, 0, E[(i + j) % len(E)]) if (i + j) % 2 else (0, y, x, E[(i + j) % len(E)]))
    return rows


def cases(pr):
    """[(case id, op, operands, expected)] for one prime."""
    p = pr.p
    Rinv = pow(FC.M128, -1, p)
    E = FC.edge_words(p)
    Ec = FC.canonical(E, p)
    out = []
    for a in E:
        for b in Ec:
            exp = a * b * Rinv % p
            out.append(("cios", (a, b), exp))
            out.append(("ps", (a, b), exp))
        out.append(("redc", (a,), a * Rinv % p))
        out.append(("canf", (a,), a % p))
        if pr.big:
            out.append(("cant", (a,), a % p))
    for a in Ec:
        for b in Ec:
            out.append(("add", (a, b), (a + b) % p))
            out.append(("sub", (a, b), (a - b) % p))
    for x, y, u, v in dot2_rows(pr):
        out.append(("dot2", (x, y, u, v), (x * y + u * v) * Rinv % p))
    return out


def test_prime_table():
    assert [pr.id for pr in FC.PRIMES] == ["test", "max128", "min_big", "m127", "m89", "two_limb", "one_limb",
                                           "three"]
    for pr in FC.PRIMES:
        assert FC.is_probable_prime(pr.p) and 3 <= pr.p < FC.M128
        assert pr.r == FC.M128 % pr.p and pr.r * pr.rinv % pr.p == 1
        assert pr.big == (pr.p > 2 ** 127)
    big = {pr.id for pr in FC.PRIMES if pr.big}
    assert big == {"test", "max128", "min_big"}
    assert 3 * FC.BY_ID["max128"].p > 2 ** 129 > 3 * FC.BY_ID["test"].p
    n0 = lambda p: (-pow(p, -1, 2 ** 32)) % 2 ** 32  # noqa: E731
    assert n0(FC.BY_ID["m127"].p) == 1 == n0(FC.BY_ID["m89"].p) and n0(FC.BY_ID["test"].p) != 1


@pytest.mark.parametrize("pid", FC.PRIME_IDS)
def test_edge_words(pid):
    pr = FC.BY_ID[pid]
    E = FC.edge_words(pr.p)
    assert E == sorted(set(E)) and all(0 <= v < FC.M128 for v in E) and 30 <= len(E) <= 64
    for v in (0, 1, 2, pr.p - 1, pr.p, pr.p + 1, 2 * pr.p, pr.kmax * pr.p, FC.MASK128, FC.M128 - pr.p, 1 << 127,
              pr.r, pr.r2, pr.rinv, pr.p - pr.rinv, 0xFFFFFFFF << 96, (1 << 96) - 1, *FC.UNIFORM_WORDS):
        assert v in E or v >= FC.M128, hex(v)  # 2p is clipped on the BIG primes


@pytest.mark.parametrize("pid", FC.PRIME_IDS)
def test_coverage_predicates(pid):
    """The operands reach what the tests exist for (Python ints only)."""
    pr = FC.BY_ID[pid]
    p = pr.p
    E = FC.edge_words(p)
    Ec = FC.canonical(E, p)
    Rinv = pow(FC.M128, -1, p)
    prods = {a * b * Rinv % p for a in E for b in Ec}
    assert 0 in prods and p - 1 in prods
    FC.assert_noncanonical(pr, E)
    FC.assert_dot2_coverage(pr, dot2_rows(pr))
    if pr.big:  # a + b of canonical values needs the 129th bit only for p > 2^127
        assert FC.sum_coverage(pr, [(a, b) for a in Ec for b in Ec]) > 0
    else:
        assert FC.sum_coverage(pr, [(a, b) for a in Ec for b in Ec]) == 0
    if 3 * p > 2 * FC.M128:
        # a Montgomery product whose pre-subtract value (a b + m p) / 2^128 < 2p needs the 129th bit.
        # Asked only for p > 2/3 2^128 (max128), where [2^128, 2p) is more than half of [0, 2p); on
        # min_big that window is 58 values wide and no fixed grid lands in it (mod_add's 129-bit sums,
        # asserted above, drive reduce_once's hi on every BIG prime).
        pinv = pow(p, -1, FC.M128)
        assert any((a * b + (-a * b * pinv) % FC.M128 * p) >> 256 for a in E for b in Ec)


@pytest.mark.parametrize("pid", FC.PRIME_IDS)
def test_field_hpp_matches_python_ints(binary, pid):
    pr = FC.BY_ID[pid]
    cs = cases(pr)
    lines = ["%s %x %s" % (op, pr.p, " ".join("%x" % v for v in args)) for op, args, _ in cs]
    got = run_lines(binary, lines)
    bad = [(op, [hex(a) for a in args], hex(g), hex(e)) for (op, args, e), g in zip(cs, got) if g != e]
    assert not bad, "%d of %d differ on %s; by op %s; first: %r" % (
        len(bad), len(cs), pid, sorted({b[0] for b in bad}), bad[:3])
    # the two Montgomery products agree with each other as well (same lines, same order)
    cios = [g for (op, _, _), g in zip(cs, got) if op == "cios"]
    ps = [g for (op, _, _), g in zip(cs, got) if op == "ps"]
    E = FC.edge_words(pr.p)
    assert cios == ps and len(cios) == len(E) * len(FC.canonical(E, pr.p))


def test_driver_rejects_bad_lines(binary):
    for text in ("cios 4 1 1\n", "nope 7 1 1\n", "redc 7\n", "dot2 7 1 1 1\n", "cios 7 1 zz\n"):
        r = subprocess.run([binary], input=text, capture_output=True, text=True, timeout=60, env=_ENV)
        assert r.returncode == 2, text
