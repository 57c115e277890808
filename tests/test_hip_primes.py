"""Every field kernel on every prime of tests/field_cases.py -- the control,
2^128 - 159 (dot2_redc's second top-limb bit), 2^127 + 29, 2^127 - 1 and
2^89 - 1 (n0 == 1), primes of two and one limbs, and 3 -- on the edge grid
E x E of carry-chain operands, bit-exact against the plain Python-int
reference AND the C oracle (which must agree with each other; the oracle
itself is pinned on the CPU by tests/test_oracle_primes.py).

This launches the BIG and the !BIG instantiation of every arithmetic kernel
(K_RV, K_MASK, recombine, verify, the codecs, K_CONV, K_ODO_PRE, open,
K_ODO_POST, the fused open + post, the wire-fused and segmented kernels, the
party session, the synthetic inputs; the batch and session kernels:
k_rv_b64_seg / k_mask_b64_seg / k_mask_json_seg, k_conv_json_seg,
k_open_post_seg behind the parties session's exchange decode, and the client
session's k_acc_b64 with k_mask_sums and K_RV over its running sums, and the
K-secret session's segmented k_acc_b64 with k_mask_sums_seg and k_rv_seg over
sums packed on the word table -- tests/field_cases.py BIG_KERNELS and
FP_KERNELS name the test for each), pins the device lowering of
addc / subc / macc96 (mont_mul_ps runs in the wire kernels and for K_MASK's
secret product, mont_mul_cios in K_RV: both are compared with the same
reference), and sends partner diffs with raw magnitudes (>= p, negative zero,
negative p, 2^128 - 1).  Each test asserts its coverage predicates on the
inputs (Python ints only) before it calls the library.  Arrays hold at most
|E|^2 (about 2.5k) words.
"""
import base64
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import coracle  # noqa: E402
from tests import field_cases as FC  # noqa: E402

NF = 0x7F7F7F7F7F7F7F7F


class Env:
    def __init__(self, pid):
        import torch
        assert torch.cuda.is_available()
        import amphora_amd as A
        self.pr = FC.BY_ID[pid]
        self.ctx = A.Context(self.pr.p, self.pr.r, self.pr.rinv)
        self.F = coracle.Field(self.pr.p, self.pr.r, self.pr.rinv, threads=4)
        self._rv = {}

    def rv(self, n):
        """(rows, the parties' arrays, expected secrets (W, 16)): the Python
        reference and the C oracle agree, computed once per party count."""
        if n not in self._rv:
            rows = FC.odo_rows(self.pr.id, n)
            odos = FC.odo_arrays(rows)
            ys, ff = FC.recombine_verify(self.pr, rows.odos)
            oy, off = self.F.recombine_verify(odos)
            assert ff == off == -1 and ys == list(rows.ys) == FC.ints(oy)
            oy.setflags(write=False)
            self._rv[n] = (rows, odos, oy)
        return self._rv[n]

    def secrets(self, W):
        E = FC.edge_words(self.pr.p)
        return [E[(3 * i + i // len(E)) % len(E)] for i in range(W)]  # raw words, >= p included


@pytest.fixture(scope="module", params=FC.PRIME_IDS)
def env(request):
    return Env(request.param)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev_odos(odos):
    return [tuple(dev(f) for f in o) for o in odos]


def host(t):
    return t.cpu().numpy()


def verdict(ff):
    """A host verdict as it is, a device verdict word as -1 / index."""
    if isinstance(ff, int):
        return ff
    import torch
    torch.cuda.synchronize()
    v = int(ff.item())
    return -1 if v == NF else v


def texts_of(odos):
    return [[base64.b64encode(np.ascontiguousarray(f).tobytes()) for f in o] for o in odos]


def dev_texts(texts):
    import torch
    return [[torch.frombuffer(bytearray(t), dtype=torch.uint8).cuda() for t in o] for o in texts]


def data_text(words16) -> bytes:
    """Jackson's compact MaskedInput "data" array of the given 16-byte words."""
    return json.dumps([{"value": base64.b64encode(bytes(w)).decode()} for w in words16],
                      separators=(",", ":")).encode()


def jackson_text(signed_pairs) -> bytes:
    return ("[" + ",".join('{"a":%d,"b":%d}' % ab for ab in signed_pairs) + "]").encode()


# ---- K_RV / K_MASK / recombine / verify --------------------------------------------
@pytest.mark.parametrize("n", FC.PARTY_COUNTS)
def test_recombine_verify(env, n):
    rows, odos, oy = env.rv(n)
    FC.rv_coverage(env.pr, rows)
    for mode in ("host", "device"):
        arrays = odos if mode == "host" else dev_odos(odos)
        y, ff = env.ctx.recombine_verify(arrays)
        assert verdict(ff) == -1, mode
        assert np.array_equal(y if mode == "host" else host(y), oy), mode
        for at in FC.fault_positions(rows.W):
            bad = FC.with_fault(odos, at)
            y, ff = env.ctx.recombine_verify(bad if mode == "host" else dev_odos(bad))
            assert verdict(ff) == at, (mode, at)
            assert np.array_equal(y if mode == "host" else host(y), oy), (mode, at)  # written for every word


@pytest.mark.parametrize("n", FC.PARTY_COUNTS)
def test_mask_input(env, n):
    pr = env.pr
    rows, odos, _ = env.rv(n)
    W = rows.W
    secrets = env.secrets(W)
    FC.assert_noncanonical(pr, secrets)
    exp = FC.mask_words(pr, secrets, rows.ys)
    om, off = env.F.mask_input(FC.arr(secrets), odos)
    assert off == -1 and FC.ints(om) == exp
    # K_MASK's secret product is the product-scanning form: one equal to 0 and one to p - 1
    prods = {s * pr.r2 * pow(FC.M128, -1, pr.p) % pr.p for s in secrets}
    assert 0 in prods and pr.p - 1 in prods
    sec = FC.arr(secrets)
    S = W - 37  # a verify-only tail of 37 mask words
    for mode in ("host", "device"):
        d = (lambda a: a) if mode == "host" else dev
        h = (lambda a: a) if mode == "host" else host
        arrays = odos if mode == "host" else dev_odos(odos)
        out, ff = env.ctx.mask_input(arrays, d(sec))
        assert verdict(ff) == -1 and np.array_equal(h(out), om), mode
        out, ff = env.ctx.mask_input(arrays, d(sec[:S]))
        assert verdict(ff) == -1 and np.array_equal(h(out), om[:S]), mode
        for at in FC.fault_positions(W):  # the last one lies in the verify-only tail
            bad = FC.with_fault(odos, at)
            out, ff = env.ctx.mask_input(bad if mode == "host" else dev_odos(bad), d(sec[:S]))
            assert verdict(ff) == at, (mode, at)


@pytest.mark.parametrize("n", FC.PARTY_COUNTS)
def test_recombine_then_verify_columns(env, n):
    rows, odos, _ = env.rv(n)
    cols = []
    for k, col in enumerate((rows.ys, rows.rs, rows.vs, rows.ws, rows.us)):
        exp = env.F.recombine([o[k] for o in odos])
        assert FC.ints(exp) == list(col)
        got = env.ctx.recombine([o[k] for o in odos])
        assert np.array_equal(got, exp), k
        assert np.array_equal(host(env.ctx.recombine([dev(o[k]) for o in odos])), exp), k
        cols.append(got)
    y, r, v, w, u = cols
    assert env.ctx.verify(y, r, u, v, w) == -1
    assert verdict(env.ctx.verify(*[dev(x) for x in (y, r, u, v, w)])) == -1
    for at in FC.fault_positions(rows.W):
        wrong = FC.arr([(x + 1) % env.pr.p if i == at else x for i, x in enumerate(rows.ws)])
        assert env.ctx.verify(y, r, u, v, wrong) == at
        wrong_u = FC.arr([(x + 1) % env.pr.p if i == at else x for i, x in enumerate(rows.us)])
        assert env.ctx.verify(y, r, wrong_u, v, w) == at


# ---- codecs ------------------------------------------------------------------------
def test_codecs(env):
    pr = env.pr
    E = FC.edge_words(pr.p)
    FC.assert_noncanonical(pr, E)
    a = FC.arr(E)
    assert FC.ints(env.ctx.to_gfp(a)) == [FC.to_gfp(pr, x % pr.p) for x in E]
    assert FC.ints(env.ctx.from_gfp(a)) == [FC.from_gfp(pr, x) for x in E]
    assert FC.ints(host(env.ctx.to_gfp(dev(a)))) == [FC.to_gfp(pr, x % pr.p) for x in E]
    assert FC.ints(host(env.ctx.from_gfp(dev(a)))) == [FC.from_gfp(pr, x) for x in E]
    secrets = [s for s in E for _ in E]
    masks = [m for _ in E for m in E]
    exp = FC.mask_words(pr, secrets, masks)
    assert FC.ints(env.ctx.mask_words(FC.arr(secrets), FC.arr(masks))) == exp
    assert FC.ints(host(env.ctx.mask_words(dev(FC.arr(secrets)), dev(FC.arr(masks))))) == exp


# ---- K_CONV --------------------------------------------------------------------------
@pytest.mark.parametrize("zero", [False, True])
def test_convert_share(env, zero):
    pr = env.pr
    E = FC.edge_words(pr.p)
    L = len(E)
    masked = [E[i // L] for i in range(L * L)]
    tuples = [(E[i % L], E[(i // L + 2 * i + 1) % L]) for i in range(L * L)]
    for col in (masked, [t[0] for t in tuples], [t[1] for t in tuples]):
        FC.assert_noncanonical(pr, col)
    m16 = FC.arr(masked)
    tup = FC.arr([x for t in tuples for x in t], 32)
    text = data_text(m16)
    for key in (0, 1, pr.p - 1, FC.UNIFORM_WORDS[0] % pr.p):
        exp = env.F.convert_share(m16, tup, key, zero)
        assert FC.ints(exp) == [x for t in FC.convert_share(pr, masked, tuples, key, zero) for x in t]
        assert np.array_equal(env.ctx.convert_share(m16, tup, key, zero), exp), key
        assert np.array_equal(host(env.ctx.convert_share(dev(m16), dev(tup), key, zero)), exp), key
        assert np.array_equal(env.ctx.convert_share_json(text, tup, key, zero), exp), key
        out, bad = env.ctx.convert_share_json(dev(np.frombuffer(text, np.uint8).copy()), dev(tup), key, zero)
        assert verdict(bad) == -1 and np.array_equal(host(out), exp), key


# ---- party kernels ---------------------------------------------------------------------
def post_arrays(rows):
    ys, m1s, m2s, _ = rows.own
    W = rows.W
    masks = FC.arr([x for i in range(W) for x in (m1s[i], 1, m2s[i], 2)], 32)
    trip = FC.arr([x for a, b, c in rows.triples for x in (a, 3, b, 4, c, 5)], 96)
    return masks, trip


def test_odo_pre(env):
    pr = env.pr
    rows = FC.post_rows(pr.id, 2)
    ys, m1s, m2s, own = rows.own
    masks, trip = post_arrays(rows)
    for col in (ys, m1s, m2s, [t[0] for t in rows.triples], [t[1] for t in rows.triples]):
        FC.assert_noncanonical(pr, col)
    assert any(d < 0 for pair in own for d in pair) and any(d > 0 for pair in own for d in pair)
    assert any(d == 0 for pair in own for d in pair)
    for stride in (16, 32):
        share = FC.arr([x for y in ys for x in ([y] if stride == 16 else [y, FC.MASK128 - y])], stride)
        exp = env.F.odo_pre(share, stride, masks, trip)
        assert FC.ints(exp[0]) == list(ys) and FC.ints(exp[1]) == list(m1s) and FC.ints(exp[2]) == list(m2s)
        assert FC.signed_of(exp[3], exp[4]) == list(own)
        got = env.ctx.odo_pre(share, stride, masks, trip)
        for g, e in zip(got, exp):
            assert np.array_equal(g, e), stride
        got = env.ctx.odo_pre(dev(share), stride, dev(masks), dev(trip))
        for g, e in zip(got, exp):
            assert np.array_equal(host(g), e), stride


@pytest.mark.parametrize("n", FC.PARTY_COUNTS)
def test_open_and_post(env, n):
    pr = env.pr
    rows = FC.post_rows(pr.id, n)
    W = rows.W
    masks, trip = post_arrays(rows)
    own_mag, own_neg = FC.signed_arrays(signed_pairs=rows.own[3])
    mags, negs = [own_mag], [own_neg]
    for pm, pg in rows.partners:
        m, g = FC.signed_arrays(mags=pm, negs=pg)
        mags.append(m)
        negs.append(g)
    opened_py = FC.post_opened(pr, rows)
    # -- coverage, on the inputs alone ---------------------------------------------------
    if n >= 2:
        flat = [x for pm, _ in rows.partners for pair in pm for x in pair]
        FC.assert_noncanonical(pr, flat)
        first = list(zip(*rows.partners[0]))
        assert ((0, 0), (1, 1)) in first and ((pr.p, pr.p), (1, 1)) in first  # negative zero, negative p
        assert FC.MASK128 in flat
    assert opened_py[0] == (pr.p - 1, pr.p - 1) and rows.triples[0][:2] == (FC.MASK128, FC.MASK128)
    # dot2_redc: 0 / 1 / 2 subtracts everywhere, hi == 2 where 3p > 2^129 (max128), on a
    # non-player-0 row (player 0's second operand b + [E] is reduced below p)
    cov = FC.assert_dot2_coverage(pr, FC.post_dot2_rows(pr, rows, opened_py, False))
    assert (cov["hi2"] > 0) == (pr.id == "max128")
    # -- reference: Python ints and the C oracle agree -------------------------------------
    opened = env.F.recombine_diffs(mags, negs)
    o = FC.ints(opened)
    assert list(zip(o[0::2], o[1::2])) == opened_py
    assert np.array_equal(env.ctx.open_diffs(mags, negs), opened)
    assert np.array_equal(host(env.ctx.open_diffs([dev(m) for m in mags], [dev(g) for g in negs])), opened)
    for p0 in (True, False):
        ew, eu = env.F.odo_post(opened.reshape(2 * W, 32), trip, p0)
        pw, pu = FC.post_expected(pr, rows, opened_py, p0)
        assert FC.ints(ew) == pw and FC.ints(eu) == pu
        w, u = env.ctx.odo_post(opened, trip, p0)
        assert np.array_equal(w, ew) and np.array_equal(u, eu), p0
        w, u = env.ctx.odo_post(dev(opened), dev(trip), p0)
        assert np.array_equal(host(w), ew) and np.array_equal(host(u), eu), p0
        w, u = env.ctx.open_post(mags, negs, trip, p0)
        assert np.array_equal(w, ew) and np.array_equal(u, eu), p0
        w, u = env.ctx.open_post([dev(m) for m in mags], [dev(g) for g in negs], dev(trip), p0)
        assert np.array_equal(host(w), ew) and np.array_equal(host(u), eu), p0


# ---- wire-fused (the mont_mul_ps kernels) -----------------------------------------------
# 1, 3, 5 and, since below 2^127 the wire kernels are templated for 1..2 parties only (3 and 5 both
# take the run-time loop there), 2 for the templated multi-party !BIG form and 4 for the BIG one
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
def test_wire_fused(env, n):
    rows, odos, oy = env.rv(n)
    FC.rv_coverage(env.pr, rows)
    W = rows.W
    secrets = env.secrets(W)
    sec = FC.arr(secrets)
    om, _ = env.F.mask_input(sec, odos)
    assert FC.ints(om) == FC.mask_words(env.pr, secrets, rows.ys)
    records = [base64.b64encode(w.tobytes()) for w in om]
    texts = texts_of(odos)
    for mode in ("host", "device"):
        d = (lambda a: a) if mode == "host" else dev
        h = (lambda a: a) if mode == "host" else host
        tx = texts if mode == "host" else dev_texts(texts)
        y, ff, bad = env.ctx.recombine_verify_b64(tx, W)
        assert verdict(ff) == -1 and verdict(bad) == -1 and np.array_equal(h(y), oy), mode
        m16, rec, ff, bad = env.ctx.mask_input_b64(tx, W, d(sec), records=True, raw=True)
        assert verdict(ff) == -1 and verdict(bad) == -1 and np.array_equal(h(m16), om), mode
        assert [r.tobytes() for r in h(rec)] == records, mode
        text, ff, bad = env.ctx.mask_input_json(tx, W, d(sec))
        assert verdict(ff) == -1 and verdict(bad) == -1, mode
        assert (text if mode == "host" else host(text).tobytes()) == data_text(om), mode
        for at in FC.fault_positions(W):
            bt = texts_of(FC.with_fault(odos, at))
            bt = bt if mode == "host" else dev_texts(bt)
            y, ff, bad = env.ctx.recombine_verify_b64(bt, W)
            assert verdict(ff) == at and verdict(bad) == -1 and np.array_equal(h(y), oy), (mode, at)
            _, _, ff, bad = env.ctx.mask_input_b64(bt, W, d(sec))
            assert verdict(ff) == at and verdict(bad) == -1, (mode, at)
            _, ff, bad = env.ctx.mask_input_json(bt, W, d(sec))
            assert verdict(ff) == at and verdict(bad) == -1, (mode, at)


# ---- segmented ----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])  # every templated form of k_rv_seg / k_mask_seg and the run-time one
def test_packed(env, n):
    """The same rows as a few objects of unequal length; a fault in the first
    and in the last object; one verdict per object."""
    import torch
    rows, odos, oy = env.rv(n)
    W = rows.W
    secrets = env.secrets(W)
    sec = FC.arr(secrets)
    om, _ = env.F.mask_input(sec, odos)
    offsets = np.array([0, 1, 130, W // 2 + 3, W - 2, W], np.uint64)
    K = len(offsets) - 1
    clean = [-1] * K
    bad = FC.with_fault(FC.with_fault(odos, 0), W - 1)
    faulty = [0, -1, -1, -1, 1]
    # the reference's per-object verdicts: each object verified on its own
    for k in range(K):
        lo, hi = int(offsets[k]), int(offsets[k + 1])
        _, off = env.F.recombine_verify([tuple(f[lo:hi] for f in o) for o in bad])
        assert off == faulty[k]
        assert FC.recombine_verify(env.pr, [tuple(FC.ints(f[lo:hi]) for f in o) for o in bad])[1] == faulty[k]
    for arrays, want in ((odos, clean), (bad, faulty)):
        y, ff = env.ctx.recombine_verify_packed(arrays, offsets)
        assert ff.tolist() == want and np.array_equal(y, oy)
        m, ff = env.ctx.mask_input_packed(arrays, offsets, sec)
        assert ff.tolist() == want and np.array_equal(m, om)
        y, ff = env.ctx.recombine_verify_packed(dev_odos(arrays), offsets)
        torch.cuda.synchronize()
        assert [(-1 if v == NF else v) for v in host(ff).tolist()] == want and np.array_equal(host(y), oy)
        m, ff = env.ctx.mask_input_packed(dev_odos(arrays), offsets, dev(sec))
        torch.cuda.synchronize()
        assert [(-1 if v == NF else v) for v in host(ff).tolist()] == want and np.array_equal(host(m), om)


# ---- party session ----------------------------------------------------------------------------
def party_inputs(pr, j, W):
    """Party j's share / mask / triple words on the grid, each party at its own stride."""
    E = FC.edge_words(pr.p)
    L = len(E)
    ys = [E[(i * (j + 1) + 2 * j) % L] for i in range(W)]
    m1s = [E[(i // L + (3 + j) * i + j) % L] for i in range(W)]
    m2s = [E[((7 + 2 * j) * i + 2) % L] for i in range(W)]
    triples = [(E[(k // L + j) % L], E[(k + 5 * j) % L], E[(k // L + 2 * k + 1 + j) % L]) for k in range(2 * W)]
    # pair 0 carries the largest magnitudes: d = (p - 1) - 0 and e = 0 - (p - 1)  (fromGfp(p - R) = p - 1)
    ys[0], m1s[0] = pr.p - pr.r, 0
    triples[0] = (0, pr.p - pr.r, triples[0][2])
    return ys, m1s, m2s, triples


@pytest.mark.parametrize("n", [2, 3])
def test_party_session(env, n):
    pr = env.pr
    L = len(FC.edge_words(pr.p))
    W = L * L // 2
    ins = [party_inputs(pr, j, W) for j in range(n)]
    own = [FC.odo_pre(pr, *ins[j]) for j in range(n)]
    mags = [x for o in own for pair in o for x in map(abs, pair)]
    assert max(mags) == pr.p - 1  # the longest decimal magnitude the text can carry
    if pr.id == "max128":
        assert len(str(max(mags))) == 39
    arrays = []
    for j in range(n):
        ys, m1s, m2s, triples = ins[j]
        share = FC.arr([x for y in ys for x in (y, FC.MASK128 - y)], 32)
        masks = FC.arr([x for i in range(W) for x in (m1s[i], 1, m2s[i], 2)], 32)
        trip = FC.arr([x for a, b, c in triples for x in (a, 3, b, 4, c, 5)], 96)
        arrays.append((share, masks, trip))
    pre = [env.F.odo_pre(a[0], 32, a[1], a[2]) for a in arrays]
    for j in range(n):
        assert FC.signed_of(pre[j][3], pre[j][4]) == own[j]
    sessions, texts = [], []
    for j in range(n):
        s = env.ctx.party_begin(arrays[j][0], 32, arrays[j][1], arrays[j][2], n)
        assert FC.ints(s.y) == ins[j][0] and FC.ints(s.r) == ins[j][1] and FC.ints(s.v) == ins[j][2]
        t = s.text()
        assert t == jackson_text(own[j])
        sessions.append(s)
        texts.append(t)
    for j, s in enumerate(sessions):
        others = [k for k in range(n) if k != j]
        for slot, k in enumerate(others, start=1):
            s.partner(slot, texts[k])
        flat = [[x for pair in own[k] for x in pair] for k in [j] + others]
        o = FC.open_values(pr, flat)
        opened = list(zip(o[0::2], o[1::2]))
        z = [FC.post_word(pr, D, E, t, j == 0) for (D, E), t in zip(opened, ins[j][3])]
        ow, ou = env.F.odo_post(env.F.recombine_diffs([pre[k][3] for k in [j] + others],
                                                      [pre[k][4] for k in [j] + others]), arrays[j][2], j == 0)
        assert FC.ints(ow) == z[0::2] and FC.ints(ou) == z[1::2]
        if j == n - 1:
            got = s.finish_b64(j == 0)
            assert got == [base64.b64encode(x.tobytes()) for x in (pre[j][0], pre[j][1], pre[j][2], ow, ou)]
        else:
            w, u = s.finish(j == 0)
            assert np.array_equal(w, ow) and np.array_equal(u, ou)
        s.close()


# ---- many requests in one parties session (k_open_post_seg behind the exchange decode) ------------------
@pytest.mark.parametrize("n", [2, 3])
def test_party_sessions(env, n):
    """test_party_session's inputs cut into requests of 1, 63, 1, 64 and the
    rest of the words: 126, 128 and more than 128 pairs against the 128-pair
    tile.  Every party on the host calls; at n = 2 on the device calls too."""
    import torch
    pr = env.pr
    L = len(FC.edge_words(pr.p))
    W = L * L // 2
    woff = np.array([0, 1, 64, 65, 129, W], np.uint64)
    cuts = [(int(a), int(b)) for a, b in zip(woff, woff[1:])]
    assert [b - a for a, b in cuts[:4]] == [1, 63, 1, 64] and W - 129 > 64
    ins = [party_inputs(pr, j, W) for j in range(n)]
    own = [FC.odo_pre(pr, *ins[j]) for j in range(n)]
    mags = [x for o in own for pair in o for x in map(abs, pair)]
    assert max(mags) == pr.p - 1  # the longest decimal magnitude the text can carry ...
    assert all(max(map(abs, o[0])) == pr.p - 1 for o in own)  # ... in the first request, of every party
    if pr.id == "max128":
        assert len(str(max(mags))) == 39
    arrays = []
    for j in range(n):
        ys, m1s, m2s, triples = ins[j]
        share = FC.arr([x for y in ys for x in (y, FC.MASK128 - y)], 32)
        masks = FC.arr([x for i in range(W) for x in (m1s[i], 1, m2s[i], 2)], 32)
        trip = FC.arr([x for a, b, c in triples for x in (a, 3, b, 4, c, 5)], 96)
        arrays.append((share, masks, trip))
    pre = [env.F.odo_pre(a[0], 32, a[1], a[2]) for a in arrays]
    want_texts, want_wu, want_fields = [], [], []
    for j in range(n):
        assert FC.signed_of(pre[j][3], pre[j][4]) == own[j]
        want_texts.append([jackson_text(own[j][2 * a:2 * b]) for a, b in cuts])
        others = [k for k in range(n) if k != j]
        flat = [[x for pair in own[k] for x in pair] for k in [j] + others]
        o = FC.open_values(pr, flat)
        z = [FC.post_word(pr, D, E, t, j == 0) for (D, E), t in zip(zip(o[0::2], o[1::2]), ins[j][3])]
        ow, ou = env.F.odo_post(env.F.recombine_diffs([pre[k][3] for k in [j] + others],
                                                      [pre[k][4] for k in [j] + others]), arrays[j][2], j == 0)
        assert FC.ints(ow) == z[0::2] and FC.ints(ou) == z[1::2]
        want_wu.append((ow, ou))
        five = [FC.arr(ins[j][0]), FC.arr(ins[j][1]), FC.arr(ins[j][2]), ow, ou]
        want_fields.append([[base64.b64encode(x[a:b].tobytes()) for x in five] for a, b in cuts])
    sessions = [env.ctx.parties_begin(arrays[j][0], 32, arrays[j][1], arrays[j][2], woff, n) for j in range(n)]
    for j, s in enumerate(sessions):
        assert FC.ints(s.y) == ins[j][0] and FC.ints(s.r) == ins[j][1] and FC.ints(s.v) == ins[j][2]
        assert s.texts() == want_texts[j], j
    for j, s in enumerate(sessions):
        for slot, k in enumerate([k for k in range(n) if k != j], start=1):
            assert (s.partner(slot, want_texts[k]) == -1).all(), (j, k)
        if j == n - 1:
            fields, rej = s.finish_b64(j == 0)
            assert not rej.any() and s.split_fields(fields) == want_fields[j]
        else:
            w, u = s.finish(j == 0)
            assert np.array_equal(w, want_wu[j][0]) and np.array_equal(u, want_wu[j][1]), j
        s.close()
    if n != 2:
        return
    dins = [tuple(dev(x) for x in a) for a in arrays]
    sessions = [env.ctx.parties_begin_dev(dins[j][0], 32, dins[j][1], dins[j][2], woff, n, want_yrv=True)
                for j in range(n)]
    texts = [s.text_dev() for s in sessions]
    bads, fields = [], []
    for j, s in enumerate(sessions):
        for slot, k in enumerate([k for k in range(n) if k != j], start=1):
            bads.append(s.partner(slot, texts[k][0], texts[k][2]))
        fields.append(s.finish_b64(j == 0))
    torch.cuda.synchronize()
    assert all((host(b) == NF).all() for b in bads)
    for j, s in enumerate(sessions):
        assert s.texts() == want_texts[j], j
        assert FC.ints(host(s.y)) == ins[j][0] and FC.ints(host(s.r)) == ins[j][1] and FC.ints(host(s.v)) == ins[j][2]
        assert s.split_fields([host(f) for f in fields[j]]) == want_fields[j], j
        s.close()


# ---- the client session: one party at a time into running sums (k_acc_b64, k_mask_sums, K_RV at n = 1) ----
@pytest.mark.parametrize("n", FC.PARTY_COUNTS)
def test_client_session(env, n):
    """The rows of test_recombine_verify as base64 texts, accumulated forward,
    in reverse and in one fixed permutation.  On the three BIG primes the
    read-modify-write add carries past 2^128; on all eight a running sum lands
    exactly on p and on p - 1, and the first and the last party to arrive bring
    words >= p in every field (asserted on the inputs below).  Host mode runs
    all three orders, device mode the permutation only: with three orders in
    both modes a parameter took 0.03-0.06 s at 3-5 parties against the 0.01-0.02 s
    of test_wire_fused's on the same rows, more than the twice it may."""
    pr = env.pr
    rows, odos, oy = env.rv(n)
    W = rows.W
    orders = FC.session_orders(n)
    covs = [FC.assert_session_coverage(pr, rows, order) for order in orders]
    cols = (rows.ys, rows.rs, rows.vs, rows.ws, rows.us)
    secrets = env.secrets(W)
    sec = FC.arr(secrets)
    om, off = env.F.mask_input(sec, odos)
    assert off == -1 and FC.ints(om) == FC.mask_words(pr, secrets, rows.ys)
    records = b"".join(base64.b64encode(w.tobytes()) for w in om)
    S = W - 193  # a verify-only tail longer than one 192-word tile
    assert 0 < S
    texts = texts_of(odos)
    by_mode = {"host": (texts, sec), "device": (dev_texts(texts), dev(sec))}
    h = lambda x: x if isinstance(x, (np.ndarray, bytes)) else host(x)  # noqa: E731

    def fed(mode, tx, order):
        s = env.ctx.client_begin(W, n) if mode == "host" else env.ctx.client_begin_dev(W, n)
        assert [verdict(s.party(j, tx[j])) for j in order] == [-1] * n
        return s

    sums = FC.running_sums(pr, rows, orders[0])  # (a sum mod p: tests/test_session_cases_cpu.py holds every order to it)
    for q, (order, cov) in enumerate(zip(orders, covs)):
        picks = {0, W - 1}
        if n >= 2:
            picks.add(cov["exact_p_at"])
        if pr.big and n >= 2:
            picks.add(cov["carry_at"])
        # host mode in every order; device mode launches the same kernels and takes the fixed permutation alone
        for mode in ("host", "device") if order == orders[-1] else ("host",):
            tx, sc = by_mode[mode]
            tag = (mode, order)
            with fed(mode, tx, order) as s:
                y, ff, bad = s.finish_verify()
                assert verdict(ff) == -1 and verdict(bad) == -1 and np.array_equal(h(y), oy), tag
                for i in sorted(picks):
                    want = tuple(col[i] for col in cols)
                    assert want == tuple(FC.from_gfp(pr, sums[k][i]) for k in range(5))
                    assert s.word(i) == want, (tag, i)
            with fed(mode, tx, order) as s:
                m16, rec, ff, bad = s.finish_mask(sc, records=True, raw=True)
                assert verdict(ff) == -1 and verdict(bad) == -1 and np.array_equal(h(m16), om), tag
                assert h(rec).tobytes() == records, tag
            with fed(mode, tx, order) as s:
                text, ff, bad = s.finish_mask_json(sc)
                assert verdict(ff) == -1 and verdict(bad) == -1, tag
                assert (text if mode == "host" else host(text).tobytes()) == data_text(om), tag
            if q == 0 or mode == "device":  # fewer secrets than masks: the shorter output, every mask verified (below)
                with fed(mode, tx, order) as s:
                    m16, rec, ff, bad = s.finish_mask(sc[:S], records=True, raw=True)
                    assert verdict(ff) == -1 and np.array_equal(h(m16), om[:S]), tag
                    assert h(rec).tobytes() == records[:24 * S], tag
    for q, at in enumerate(FC.fault_positions(W)):  # W - 1 and W // 2 lie in the verify-only tail of `S` secrets
        order = orders[q % len(orders)]
        bt = texts_of(FC.with_fault(odos, at))
        for mode, tx, sc in (("host", bt, sec), ("device", dev_texts(bt), by_mode["device"][1])):
            with fed(mode, tx, order) as s:
                y, ff, bad = s.finish_verify()
                assert verdict(ff) == at and verdict(bad) == -1, (mode, at)
            with fed(mode, tx, order) as s:
                assert verdict(s.finish_mask(sc[:S])[2]) == at, (mode, at)
            with fed(mode, tx, order) as s:
                assert verdict(s.finish_mask_json(sc)[1]) == at, (mode, at)


# ---- many objects straight from their base64 texts (k_rv_b64_seg, k_mask_b64_seg, k_mask_json_seg) --------
def per_object(v):
    """A verdict array of either mode as a list of -1 / value."""
    if not isinstance(v, np.ndarray):
        import torch
        torch.cuda.synchronize()
        v = host(v)
    return [-1 if int(x) == NF else int(x) for x in v]


def slotted(texts_by_object, sizes, slot_chars):
    """(text offsets, per party the five field buffers): object o's own text at
    the sum of its predecessors' slots, '!' everywhere else."""
    toff = np.concatenate([[0], np.cumsum([slot_chars(w) for w in sizes])]).astype(np.uint64)
    n = len(texts_by_object[0])
    bufs = [[np.full(int(toff[-1]), ord("!"), np.uint8) for _ in range(5)] for _ in range(n)]
    for o, obj in enumerate(texts_by_object):
        for j in range(n):
            for k in range(5):
                t = np.frombuffer(obj[j][k], np.uint8)
                bufs[j][k][int(toff[o]):int(toff[o]) + t.size] = t
    return toff[:-1].copy(), bufs


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])  # every templated form and the run-time loop, BIG and !BIG
def test_wire_packed(env, n):
    """test_packed's objects, each object's fields encoded on their own (all
    three base64 paddings occur); a fault in the first and in the last
    object; one verdict per object."""
    import amphora_amd
    import torch
    pr = env.pr
    rows, odos, oy = env.rv(n)
    FC.rv_coverage(pr, rows)
    W = rows.W
    secrets = env.secrets(W)
    sec = FC.arr(secrets)
    om, _ = env.F.mask_input(sec, odos)
    assert FC.ints(om) == FC.mask_words(pr, secrets, rows.ys)
    records = np.frombuffer(b"".join(base64.b64encode(w.tobytes()) for w in om), np.uint8).reshape(W, 24)
    woff = np.array([0, 1, 130, W // 2 + 3, W - 2, W], np.uint64)
    cuts = [(int(a), int(b)) for a, b in zip(woff, woff[1:])]
    K = len(cuts)
    assert {(16 * (b - a)) % 3 for a, b in cuts} == {0, 1, 2}  # "", "==" and "=" at the texts' ends
    clean = [-1] * K
    bad = FC.with_fault(FC.with_fault(odos, 0), W - 1)
    faulty = [0, -1, -1, -1, 1]
    for k, (lo, hi) in enumerate(cuts):  # the reference's per-object verdicts: each object verified on its own
        _, off = env.F.recombine_verify([tuple(f[lo:hi] for f in o) for o in bad])
        assert off == faulty[k]
        assert FC.recombine_verify(pr, [tuple(FC.ints(f[lo:hi]) for f in o) for o in bad])[1] == faulty[k]
    want_texts = [data_text(om[lo:hi]) for lo, hi in cuts]

    def many(ff):
        if not isinstance(ff, np.ndarray):
            torch.cuda.synchronize()
            ff = host(ff)
        return [-1 if int(v) == NF else int(v) for v in ff]

    for arrays, want in ((odos, clean), (bad, faulty)):
        objs = [[[base64.b64encode(f[lo:hi].tobytes()) for f in o] for o in arrays] for lo, hi in cuts]
        toff, bufs = slotted(objs, [hi - lo for lo, hi in cuts], amphora_amd._lib.wire_slot_chars)
        for mode in ("host", "device"):
            d = (lambda a: a) if mode == "host" else dev
            g = (lambda a: a) if mode == "host" else host
            tx = [[d(f) for f in o] for o in bufs]
            wo, to = (woff, toff) if mode == "host" else (dev(woff.view(np.int64)), dev(toff.view(np.int64)))
            y, ff, bc = env.ctx.recombine_verify_b64_packed(tx, wo, to)
            assert many(ff) == want and many(bc) == clean and np.array_equal(g(y), oy), mode
            m16, rec, ff, bc = env.ctx.mask_input_b64_packed(tx, wo, to, d(sec), records=True, raw=True)
            assert many(ff) == want and many(bc) == clean, mode
            assert np.array_equal(g(m16), om) and np.array_equal(g(rec), records), mode
            text, oo, ff, bc = env.ctx.mask_input_json_packed(tx, wo, to, d(sec))
            assert many(ff) == want and many(bc) == clean, mode
            text, oo = g(text), g(oo)
            for o in range(K):
                got = text[int(oo[o]):int(oo[o]) + len(want_texts[o])].tobytes()
                assert got == want_texts[o], (mode, o)


# ---- the client session for K secrets (k_acc_b64's SEG form, k_mask_sums_seg, k_rv_seg over the sums) --------
CLIENTS_SIZES = [0, 1, 192, 193, 2, 385, 0, 3, 191]  # and one object of the remaining rows (554 of 1,521)


def clients_cut(W, witnesses):
    """The rows as ten objects: CLIENTS_SIZES and the rest.  The list is rotated
    until the witness words (a sum of exactly p, a carry out of bit 127) do not
    all lie where an object's own index equals the packed one (object 0, and
    whatever follows it at word offset 0)."""
    sizes = CLIENTS_SIZES + [W - sum(CLIENTS_SIZES)]
    assert sizes[-1] > 0  # (189 words on the prime 3, whose edge set is the smallest; 554 to 1,149 elsewhere)
    for _ in sizes:
        woff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
        first = next(int(b) for b in woff[1:] if b)  # the end of the first object that has words
        if not witnesses or any(i >= first for i in witnesses):
            return sizes, woff
        sizes = sizes[1:] + sizes[:1]
    raise AssertionError("no rotation of the sizes separates the witness words from object 0")


@pytest.mark.parametrize("n", FC.PARTY_COUNTS)
def test_clients_session(env, n):
    """test_client_session's rows as the ten objects of ONE K-secret session:
    empty objects first and inside, objects of one word, of exactly one tile, of
    one word more and of several tiles, so the per-object tiles have uneven
    prefix sums.  Host mode in all three arrival orders, device mode in the
    fixed permutation, all three finishes; secrets, masked words, records and
    the framed texts whole against Python ints and the C oracle; the sums read
    back at the first and last word and at the coverage words; one fault per
    position of FC.fault_positions: the owning object's verdict is the local
    index, every other object is clean."""
    pr = env.pr
    rows, odos, oy = env.rv(n)
    W = rows.W
    orders = FC.session_orders(n)
    covs = [FC.assert_session_coverage(pr, rows, order) for order in orders]
    witnesses = {c[name] for c in covs for name in ("exact_p_at", "carry_at") if c[name] is not None}
    assert bool(witnesses) == (n >= 2)
    sizes, woff = clients_cut(W, witnesses)
    K = len(sizes)
    cuts = [(int(a), int(b)) for a, b in zip(woff, woff[1:])]
    assert sizes.count(0) == 2 and cuts[-1][1] == W

    def owner(i):
        """(object, local index) of packed word i."""
        o = next(o for o, (lo, hi) in enumerate(cuts) if lo <= i < hi)
        return o, i - cuts[o][0]

    # the witnesses do not both lie in object 0, nor anywhere else where local and packed indices agree
    assert not witnesses or any(owner(i)[0] != 0 and cuts[owner(i)[0]][0] > 0 for i in witnesses)
    cols = (rows.ys, rows.rs, rows.vs, rows.ws, rows.us)
    sums = FC.running_sums(pr, rows, orders[0])
    secrets = env.secrets(W)
    sec = FC.arr(secrets)
    om, off = env.F.mask_input(sec, odos)
    assert off == -1 and FC.ints(om) == FC.mask_words(pr, secrets, rows.ys)
    records = np.frombuffer(b"".join(base64.b64encode(w.tobytes()) for w in om), np.uint8).reshape(W, 24)
    # the dense layouts, from the word counts alone
    chars = lambda w: 4 * ((16 * w + 2) // 3)  # noqa: E731
    toff, bufs = slotted([[[base64.b64encode(f[lo:hi].tobytes()) for f in o] for o in odos] for lo, hi in cuts], sizes,
                         lambda w: (chars(w) + 15) & ~15)
    framed = [data_text(om[lo:hi]) for lo, hi in cuts]
    uoff = np.concatenate([[0], np.cumsum([(len(t) + 15) & ~15 for t in framed])]).astype(np.uint64)
    assert [len(t) for t in framed] == [37 * w + 1 if w else 2 for w in sizes] and framed[0] == b"[]"
    want_text = np.full(int(uoff[-1]), 0xA5, np.uint8)
    for o, t in enumerate(framed):
        want_text[int(uoff[o]):int(uoff[o]) + len(t)] = np.frombuffer(t, np.uint8)
    clean = [-1] * K
    dsec = dev(sec)
    by_mode = {"host": bufs, "device": [[dev(f) for f in five] for five in bufs]}
    h = lambda x: x if isinstance(x, np.ndarray) else host(x)  # noqa: E731

    def fed(mode, tx, order):
        s = env.ctx.clients_begin(woff, n) if mode == "host" else env.ctx.clients_begin_dev(woff, n)
        assert s.field_offsets.tolist() == toff.tolist() and s.upload_offsets.tolist() == uoff[:-1].tolist()
        assert (s.field_chars, s.upload_chars) == (bufs[0][0].size, want_text.size)
        assert [per_object(s.party(j, tx[j])) for j in order] == [clean] * n
        return s

    def finished(mode, tx, order, finish):
        """-> (first_fails, bad_chars, the outputs as host arrays, the words read back)."""
        with fed(mode, tx, order) as s:
            if finish == "verify":
                y, ff, bad = s.finish_verify()
                outs = [y]
            elif finish == "mask":
                m16, rec, ff, bad = s.finish_mask(dsec if mode == "device" else sec, records=True, raw=True)
                outs = [m16, rec]
            else:
                out = np.full(want_text.size, 0xA5, np.uint8)
                text, ff, bad = s.finish_mask_json(dsec if mode == "device" else sec,
                                                   out=dev(out) if mode == "device" else out)
                outs = [text]
            ff, bad = per_object(ff), per_object(bad)
            return ff, bad, [h(x) for x in outs], {i: s.word(*owner(i)) for i in (picks if finish == "verify" else ())}

    want = {"verify": [oy], "mask": [om, records], "mask_json": [want_text]}
    for order, cov in zip(orders, covs):
        picks = {0, W - 1} | {cov[name] for name in ("exact_p_at", "carry_at") if cov[name] is not None}
        # host mode in every order; device mode launches the same kernels and takes the fixed permutation alone
        for mode in ("host", "device") if order == orders[-1] else ("host",):
            for finish in ("verify", "mask", "mask_json"):
                ff, bad, outs, words = finished(mode, by_mode[mode], order, finish)
                tag = (mode, order, finish)
                assert ff == clean and bad == clean, (tag, ff, bad)
                assert all(g.shape == w.shape and np.array_equal(g, w) for g, w in zip(outs, want[finish])), tag
                for i, got in words.items():  # the sums, at (object, local index)
                    assert got == tuple(col[i] for col in cols) == tuple(FC.from_gfp(pr, sums[k][i]) for k in range(5)), \
                        (tag, i, owner(i))
    picks = ()
    for q, at in enumerate(FC.fault_positions(W)):
        order = orders[q % len(orders)]
        o, local = owner(at)
        lo, hi = cuts[o]
        t = np.frombuffer(base64.b64encode(FC.with_fault(odos, at)[0][3][lo:hi].tobytes()), np.uint8)
        w_text = bufs[0][3].copy()  # party 0's w: the owning object's text alone changes
        assert t.size == chars(hi - lo) and not np.array_equal(w_text[int(toff[o]):int(toff[o]) + t.size], t)
        w_text[int(toff[o]):int(toff[o]) + t.size] = t
        faulty = clean[:o] + [local] + clean[o + 1:]
        for mode in ("host", "device"):
            five = list(by_mode[mode][0])
            five[3] = w_text if mode == "host" else dev(w_text)
            tx = [five] + list(by_mode[mode][1:])
            for finish in ("verify", "mask", "mask_json"):
                ff, bad, _, _ = finished(mode, tx, order, finish)
                assert ff == faulty and bad == clean, (mode, at, finish, ff, bad)


# ---- many uploads in one launch (k_conv_json_seg) ------------------------------------------------------
@pytest.mark.parametrize("zero", [False, True])
def test_convert_share_json_packed(env, zero):
    """test_convert_share's words as objects of 1, 127, 1 and the rest: both
    sides of the 128-record tile, every object with its own "data" text at
    its own alignment in one buffer."""
    import torch
    pr = env.pr
    E = FC.edge_words(pr.p)
    L = len(E)
    W = L * L
    masked = [E[i // L] for i in range(W)]
    tuples = [(E[i % L], E[(i // L + 2 * i + 1) % L]) for i in range(W)]
    for col in (masked, [t[0] for t in tuples], [t[1] for t in tuples]):
        FC.assert_noncanonical(pr, col)
    m16 = FC.arr(masked)
    tup = FC.arr([x for t in tuples for x in t], 32)
    woff = np.array([0, 1, 128, 129, W], np.uint64)
    cuts = [(int(a), int(b)) for a, b in zip(woff, woff[1:])]
    own = [data_text(m16[lo:hi]) for lo, hi in cuts]
    buf = b"!".join(own)  # one foreign byte between the texts, which so start at offsets 0, 7, 4 and 11 mod 16
    toff = np.array([sum(len(t) + 1 for t in own[:o]) for o in range(len(own))], np.uint64)
    assert len({int(t) % 16 for t in toff}) >= 3
    dbuf = dev(np.frombuffer(buf, np.uint8).copy())
    for key in (0, 1, pr.p - 1, FC.UNIFORM_WORDS[0] % pr.p):
        exp = env.F.convert_share(m16, tup, key, zero)
        for lo, hi in cuts:  # Python ints on each object alone
            assert FC.ints(exp[lo:hi]) == [x for t in FC.convert_share(pr, masked[lo:hi], tuples[lo:hi], key, zero)
                                           for x in t], (key, lo)
        out, bad = env.ctx.convert_share_json_packed(buf, woff, toff, tup, key, zero)
        assert bad.tolist() == [-1] * len(cuts) and np.array_equal(out, exp), key
        out, bad = env.ctx.convert_share_json_packed(dbuf, woff, toff, dev(tup), key, zero)
        torch.cuda.synchronize()
        assert host(bad).tolist() == [NF] * len(cuts) and np.array_equal(host(out), exp), key
        outs, bad = env.ctx.convert_share_json_batch(own, [tup[lo:hi] for lo, hi in cuts], key, zero)
        assert bad.tolist() == [-1] * len(cuts), key
        assert all(np.array_equal(o, exp[lo:hi]) for o, (lo, hi) in zip(outs, cuts)), key


# ---- device synth ---------------------------------------------------------------------------------
def test_device_synth(env):
    import torch
    pr = env.pr
    W = 2500
    as_ints = lambda od: [tuple(FC.ints(host(f)) for f in o) for o in od]  # noqa: E731
    for n, permille in ((1, 0), (3, 0), (3, 300), (16, 300)):
        odos, _, plain = env.ctx.synth_odos(seed=11 + n, n=n, words=W, noncanon_permille=permille, with_plain=True)
        torch.cuda.synchronize()
        hodos = [tuple(host(f) for f in o) for o in odos]
        oy, off = env.F.recombine_verify(hodos)
        assert off == -1 and np.array_equal(oy, host(plain)), (n, permille)
        assert FC.recombine_verify(pr, as_ints(odos)) == (FC.ints(oy), -1)
    for n, at in ((1, 0), (2, W - 1), (3, W // 2)):
        odos, _, _ = env.ctx.synth_odos(seed=7, n=n, words=W, fault_index=at)
        torch.cuda.synchronize()
        _, off = env.F.recombine_verify([tuple(host(f) for f in o) for o in odos])
        assert off == at, (n, at)
        assert FC.recombine_verify(pr, as_ints(odos))[1] == at
    words = host(env.ctx.synth_words(seed=9, count=W))
    assert all(x < pr.p for x in FC.ints(words))
    # the same counter-based generator as the oracle's: the 128-bit hash of (seed, i) mod p
    assert np.array_equal(words, env.F.synth_words(seed=9, count=W, mont=False))
