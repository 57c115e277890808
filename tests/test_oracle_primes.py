"""The C oracle (oracle/amphora_oracle.c) on every prime of
tests/field_cases.py -- the control, the largest and smallest BIG primes, the
Mersenne primes, primes of two and one limbs, and 3 -- against the Python
BigInteger restatement (oracle/amphora_oracle.py) and the plain Python-int
references of field_cases, on the edge grid E x E.  The GPU tests of
tests/test_hip_primes.py lean on this checker, so it is pinned here first.
Partner diffs take raw magnitudes from E (>= p, p, 0, 2^128 - 1) with both
signs.  Bit-exact, CPU only.
"""
import numpy as np
import pytest

from oracle import amphora_oracle as O
from oracle import coracle
from tests import field_cases as FC


@pytest.fixture(scope="module", params=FC.PRIME_IDS)
def env(request):
    pr = FC.BY_ID[request.param]
    return pr, coracle.Field(pr.p, pr.r, pr.rinv, threads=2)


def le(x):
    return int(x).to_bytes(16, "little")


@pytest.mark.parametrize("n", [1, 2, 5])
def test_recombine_and_verify(env, n):
    pr, F = env
    rows = FC.odo_rows(pr.id, n)
    FC.rv_coverage(pr, rows)
    odos = FC.odo_arrays(rows)
    util = O.ClientSecretShareUtil(pr.p, pr.r, pr.rinv)
    for k, col in enumerate((rows.ys, rows.rs, rows.vs, rows.ws, rows.us)):
        got = FC.ints(F.recombine([o[k] for o in odos]))
        assert got == list(col)
        assert got == util.recombine_object([o[k].tobytes() for o in odos])
    ys, ff = FC.recombine_verify(pr, rows.odos)
    assert ff == -1 and ys == list(rows.ys)
    y, off = F.recombine_verify(odos)
    assert off == -1 and FC.ints(y) == ys
    O.verify_output_delivery_objects(util, [O.OutputDeliveryObject(*[f.tobytes() for f in o]) for o in odos])
    for at in FC.fault_positions(rows.W):
        bad = FC.with_fault(odos, at)
        y, off = F.recombine_verify(bad)
        assert off == at and FC.ints(y) == ys
        assert FC.recombine_verify(pr, [tuple(FC.ints(f) for f in o) for o in bad])[1] == at


@pytest.mark.parametrize("n", [1, 3])
def test_mask_input(env, n):
    pr, F = env
    rows = FC.odo_rows(pr.id, n)
    E = FC.edge_words(pr.p)
    secrets = [E[(3 * i + i // len(E)) % len(E)] for i in range(rows.W)]  # raw, >= p included
    FC.assert_noncanonical(pr, secrets)
    out, ff = F.mask_input(FC.arr(secrets), FC.odo_arrays(rows))
    assert ff == -1 and FC.ints(out) == FC.mask_words(pr, secrets, rows.ys)
    util = O.ClientSecretShareUtil(pr.p, pr.r, pr.rinv)
    assert [out[i].tobytes() for i in range(0, rows.W, 7)] == \
        [util.mask_input(secrets[i], rows.ys[i]) for i in range(0, rows.W, 7)]


@pytest.mark.parametrize("zero", [False, True])
def test_convert_share(env, zero):
    pr, F = env
    E = FC.edge_words(pr.p)
    L = len(E)
    masked = [E[i // L] for i in range(L * L)]
    tuples = [(E[i % L], E[(i // L + 2 * i + 1) % L]) for i in range(L * L)]
    FC.assert_noncanonical(pr, masked)
    FC.assert_noncanonical(pr, [t[0] for t in tuples])
    FC.assert_noncanonical(pr, [t[1] for t in tuples])
    tup = FC.arr([x for t in tuples for x in t], 32)
    for key in (0, 1, pr.p - 1, FC.UNIFORM_WORDS[0] % pr.p):
        got = F.convert_share(FC.arr(masked), tup, key, zero)
        exp = FC.convert_share(pr, masked, tuples, key, zero)
        assert FC.ints(got) == [x for t in exp for x in t]


@pytest.mark.parametrize("n", [1, 2, 3, 16])
def test_output_delivery(env, n):
    """odo_pre -> recombine_diffs -> odo_post for both players, the partners'
    magnitudes raw from E (>= p, negative zero, negative p, 2^128 - 1)."""
    pr, F = env
    rows = FC.post_rows(pr.id, n)
    ys, m1s, m2s, own = rows.own
    W = rows.W
    for stride in (16, 32):
        share = FC.arr([x for y in ys for x in ([y] if stride == 16 else [y, FC.MASK128 - y])], stride)
        masks = FC.arr([x for i in range(W) for x in (m1s[i], 1, m2s[i], 2)], 32)
        trip = FC.arr([x for a, b, c in rows.triples for x in (a, 3, b, 4, c, 5)], 96)
        y, r, v, mag, neg = F.odo_pre(share, stride, masks, trip)
        assert FC.ints(y) == list(ys) and FC.ints(r) == list(m1s) and FC.ints(v) == list(m2s)
        assert FC.signed_of(mag, neg) == list(own)
    spdz = O.MpSpdzIntegrationUtils(pr.p, pr.r, pr.rinv)
    pairs = O.odo_factor_pairs(spdz, FC.arr(ys).tobytes(), O.parse_input_masks(masks.tobytes()))[3]
    assert O.beaver_diffs(spdz, pairs, O.parse_triples(trip.tobytes())) == list(own)
    mags, negs = [mag], [neg]
    for pm, pg in rows.partners:
        m, g = FC.signed_arrays(mags=pm, negs=pg)
        mags.append(m)
        negs.append(g)
    if n >= 2:
        flat = [x for pm, _ in rows.partners for pair in pm for x in pair]
        FC.assert_noncanonical(pr, flat)
        assert any(m == (0, 0) and g == (1, 1) for m, g in zip(*rows.partners[0]))        # negative zero
        assert any(m == (pr.p, pr.p) and g == (1, 1) for m, g in zip(*rows.partners[0]))  # negative p
        assert FC.MASK128 in flat
    opened = F.recombine_diffs(mags, negs)
    exp_open = FC.post_opened(pr, rows)
    got_open = FC.ints(opened)
    assert list(zip(got_open[0::2], got_open[1::2])) == exp_open
    assert exp_open[0] == (pr.p - 1, pr.p - 1)
    for p0 in (True, False):
        if not p0:  # player 0's second operand is reduced (b + [E] < p): no raw 2^128 - 1 there
            FC.assert_dot2_coverage(pr, FC.post_dot2_rows(pr, rows, exp_open, p0))
        w, u = F.odo_post(opened.reshape(2 * W, 32), trip, p0)
        ew, eu = FC.post_expected(pr, rows, exp_open, p0)
        assert FC.ints(w) == ew and FC.ints(u) == eu
        # the BigInteger restatement takes the signed, unreduced sums
        signed = FC.post_party_signed(rows)
        raw = [tuple(sum(party[k][c] for party in signed) for c in range(2)) for k in range(0, 2 * W, 97)]
        prod = [O.multiply_shared_secrets(spdz, tuple(le(t) for t in rows.triples[k]), *raw[q], 0 if p0 else 1)
                for q, k in enumerate(range(0, 2 * W, 97))]
        assert [int.from_bytes(spdz.to_gfp(z), "little") for z in prod] == \
            [(eu if k % 2 else ew)[k // 2] for k in range(0, 2 * W, 97)]


@pytest.mark.parametrize("n", [1, 2, 4])
def test_synth(env, n):
    pr, F = env
    W = 257
    odos, _ = F.synth_odos(seed=31 + n, n=n, W=W)
    as_ints = lambda od: [tuple(FC.ints(f) for f in o) for o in od]  # noqa: E731
    ys, ff = FC.recombine_verify(pr, as_ints(odos))
    assert ff == -1
    assert all(w < pr.p for o in as_ints(odos) for f in o for w in f)
    nc, _ = F.synth_odos(seed=31 + n, n=n, W=W, noncanon_permille=400)
    assert FC.recombine_verify(pr, as_ints(nc)) == (ys, -1)
    lifted = sum(1 for o in as_ints(nc) for f in o for w in f if w >= pr.p)
    if not pr.big:  # [x] + p always fits below 2^127; on max128 it fits for 158 values only
        assert lifted > 0
    plain = FC.arr(FC.edge_words(pr.p)[:W] + [0] * max(0, W - len(FC.edge_words(pr.p))))
    given, _ = F.synth_odos(seed=5, n=n, W=W, y_plain=plain)
    assert FC.recombine_verify(pr, as_ints(given)) == ([v % pr.p for v in FC.ints(plain)], -1)
    for at in (0, W // 2, W - 1):
        bad, _ = F.synth_odos(seed=31 + n, n=n, W=W, fault_index=at)
        assert FC.recombine_verify(pr, as_ints(bad)) == (ys, at)
        assert F.recombine_verify(bad)[1] == at
    plain_words = FC.ints(F.synth_words(seed=9, count=W, mont=False))
    mont_words = FC.ints(F.synth_words(seed=9, count=W, mont=True))
    assert all(x < pr.p for x in plain_words)
    assert mont_words == [FC.to_gfp(pr, x) for x in plain_words]
    if pr.p > 2 ** 32:
        assert len(set(plain_words)) > W // 2
