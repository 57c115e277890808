"""The body calls of the K-secret client session on the GPU (include/
amphora_client_bodies.h): a party's K response bodies handed in as they are,
every member decoded at whatever byte it starts -- bit for bit what
amph_clients_party gives on the gathered texts, and the C oracle's results per
object.  Nothing compares against the body calls themselves.

Shape: [0, 1, 192, 0, 0, 193, 2, 385, 3, 191, 0] as tests/test_clients_session.py
(all three paddings, both sides of a tile edge), 40 small objects, and two
objects on the eight primes.  Every field meets every residue mod 16: 16
paddings in front of the first member move all five members byte by byte.
No test provokes a fault: reads outside the granules that hold text are
excluded by the code and by tests/bodies/test_clients_bodies_cpu.py.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import bodies_cases as BC  # noqa: E402
from tests import field_cases as FC  # noqa: E402
from tests import text_cases as TC  # noqa: E402
from tests.test_clients_session import (A, Case, E_PARAM, FINISHES, NF, OK, b64, case, chars,  # noqa: E402,F401
                                        check_against_oracle, check_against_packed, ctx, ctx1, packed_reference,
                                        run_session)

ABSENT = 2 ** 64 - 1


def bodies_for(L, cs, j, pad=0, pads=None, order=(0, 1, 2, 3, 4), pretty=False, tags="plain", tags_at="first"):
    """Party j's K bodies (bytearrays) and their (K, 5) starts, as the scanner
    gives them; pads: {object: padding} over the common `pad`."""
    bodies, starts = [], np.empty((cs.K, 5), np.uint64)
    for o, W in enumerate(cs.sizes):
        p = (pads or {}).get(o, pad)
        raw = BC.body([b64(f) for f in cs.objs[o][j]], order, pretty, tags, tags_at, pad=p).encode("utf-8")
        starts[o], lens = L.bodies_scan(raw)
        assert (lens == chars(W)).all()
        bodies.append(bytearray(raw))
    return bodies, starts


def run_bodies(ctx, cs, bodies, starts, order, finish, dev=False, prefill=0xEE):
    """run_session of tests/test_clients_session.py with every party handed in
    through party_bodies: -> ({party: (status, message)}, finish's result)."""
    import torch
    s = ctx.clients_begin_dev(cs.woff, cs.n) if dev else ctx.clients_begin(cs.woff, cs.n)
    with s:
        parts = {}
        for j in order:
            parts[j] = s.party_bodies(j, [bytes(b) for b in bodies[j]], starts[j], status=not dev)
        assert s.parties_seen == cs.n
        sec = torch.from_numpy(cs.secrets).cuda() if dev else cs.secrets
        if finish == "verify":
            res = s.finish_verify(status=True)
        elif finish == "mask":
            res = s.finish_mask(sec, records=True, raw=True, status=True)
        else:
            out = np.full(max(cs.upload_chars, 1), prefill, np.uint8)
            res = s.finish_mask_json(sec, out=torch.from_numpy(out).cuda() if dev else out, status=True)
        if dev:
            torch.cuda.synchronize()
            host = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
            unf = lambda v: np.where(v == NF, -1, v)  # noqa: E731
            res = tuple(host(x) for x in res[:-3]) + (unf(host(res[-3])), unf(host(res[-2])), res[-1])
        return parts, res


def same(res, ref, status=True):
    """Bit for bit: every output array, both verdict arrays, status and message."""
    for x, r in zip(res[:-1], ref[:-1]):
        assert (x is None and r is None) or np.array_equal(x, r)
    if status:
        assert res[-1] == ref[-1], (res[-1], ref[-1])


_SLOTTED = {}


def slotted(ctx1, shape, n, finish, order):
    """amph_clients_party on the gathered texts: computed once, shared, left unchanged."""
    key = (shape, n, finish, tuple(order))
    if key not in _SLOTTED:
        cs = case(shape, n)
        _SLOTTED[key] = run_session(ctx1, cs, cs.buffers(), order, finish)[1]
    return _SLOTTED[key]


# ---- the alignment sweep ----------------------------------------------------------------------------
@pytest.mark.parametrize("pad", range(16))
def test_every_field_at_every_residue(A, ctx1, pad):
    L = A._lib
    for n in (1, 3):
        cs = case("tiles", n)
        order = list(range(n))[::-1]
        made = [bodies_for(L, cs, j, pad=pad) for j in range(n)]
        bodies, starts = [m[0] for m in made], [m[1] for m in made]
        if pad:  # one byte of padding moves every member's residue by one
            base = bodies_for(L, cs, 0)[1]
            assert ((starts[0] - base) == pad).all()
        for finish in FINISHES:
            parts, res = run_bodies(ctx1, cs, bodies, starts, order, finish)
            assert all(parts[j] == (OK, "") for j in order)
            check_against_oracle(cs, finish, res)
            same(res, slotted(ctx1, "tiles", n, finish, order))


def test_the_sweep_meets_every_residue_in_every_field(A):
    L = A._lib
    cs = case("tiles", 1)
    seen = {(o, k): set() for o in range(cs.K) for k in range(5)}
    for pad in range(16):
        _, starts = bodies_for(L, cs, 0, pad=pad)
        for (o, k) in seen:
            seen[(o, k)].add(int(starts[o, k]) % 16)
    assert all(v == set(range(16)) for v in seen.values())


# ---- other inputs --------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,kw", [("tiles", dict(order=(2, 3, 4, 0, 1), tags="names", tags_at="middle")),
                                      ("tiles", dict(order=(4, 0, 1, 2, 3), pretty=True, tags="unicode", pad=5)),
                                      ("tiles", dict(pretty=True, tags="quotes", tags_at="last", pad=11)),
                                      ("forty", dict(order=(1, 2, 3, 4, 0), tags="braces", pad=3)),
                                      ("one", dict(tags="nested", pad=9))])
def test_rotated_pretty_and_many_bodies(A, ctx, shape, kw):
    L = A._lib
    cs = case(shape, 3)
    made = [bodies_for(L, cs, j, **kw) for j in range(3)]
    bodies, starts = [m[0] for m in made], [m[1] for m in made]
    for finish in FINISHES:
        parts, res = run_bodies(ctx, cs, bodies, starts, [1, 2, 0], finish)
        assert all(parts[j] == (OK, "") for j in range(3))
        check_against_oracle(cs, finish, res)
        same(res, run_session(ctx, cs, cs.buffers(), [1, 2, 0], finish)[1])
        check_against_packed(cs, res, packed_reference(ctx, cs, cs.buffers(), finish))


def test_scan_bodies_is_the_default(A, ctx1):
    """party_bodies without starts scans in C; a member of another length is refused before any launch."""
    L = A._lib
    cs = case("tiles", 2)
    made = [bodies_for(L, cs, j, pad=7) for j in range(2)]
    with ctx1.clients_begin(cs.woff, 2) as s:
        launches = ctx1.stats()["kernel_launches"]
        odd = [bytes(b) for b in made[0][0]]
        odd[7] = odd[7].replace(b'"wShares":"', b'"wShares":"AAAA')
        with pytest.raises(L.AmphoraNativeError, match="object 7: base64 fields of") as e:
            s.party_bodies(0, odd)
        assert e.value.status == L.AMPH_E_LEN and s.parties_seen == 0
        with pytest.raises(L.BodyNotPlain):
            s.party_bodies(0, odd[:7] + [b"{}"] + odd[8:])
        past = made[0][1].copy()
        past[9, 4] = len(made[0][0][9]) - chars(191) + 1  # its last character would lie past the body
        with pytest.raises(L.AmphoraNativeError, match="object 9: uShares starts at byte") as e:
            s.party_bodies(0, [bytes(b) for b in made[0][0]], past)
        assert e.value.status == E_PARAM and s.parties_seen == 0
        assert ctx1.stats()["kernel_launches"] == launches
        for j in (1, 0):
            assert s.party_bodies(j, [bytes(b) for b in made[j][0]]) is None
        with pytest.raises(L.AmphoraNativeError, match="party 1's slot is already taken"):
            s.party_bodies(1, [bytes(b) for b in made[1][0]])
        y, ff, bad = s.finish_verify()
    assert (ff == -1).all() and (bad == -1).all() and np.array_equal(y, np.concatenate(cs.y))


@pytest.mark.parametrize("dev", [False, True])
def test_an_absent_object_between_live_ones(A, ctx1, dev):
    """Object 5 (193 words) of party 1 is absent: its verdict is what a slot of
    NUL bytes reports, its neighbours keep bytes and verdicts."""
    L = A._lib
    cs = case("tiles", 3)
    made = [bodies_for(L, cs, j, pad=13) for j in range(3)]
    bodies, starts = [m[0] for m in made], [m[1].copy() for m in made]
    starts[1][5, 2] = ABSENT  # one entry marks the object
    bodies[1][5] = bytearray(b"not even JSON")
    want = {5: 5 * 1 * chars(193)}
    zeroed = cs.buffers()
    for k in range(5):
        zeroed[1][k][int(cs.foff[5]):int(cs.foff[5]) + chars(193)] = 0
    for finish in FINISHES:
        parts, res = run_bodies(ctx1, cs, bodies, starts, [0, 1, 2], finish, dev=dev)
        ref = run_session(ctx1, cs, zeroed, [0, 1, 2], finish, dev=dev)
        if not dev:
            assert parts[1][0] == E_PARAM and parts[1][1] == ref[0][1][1][1]
            assert parts[1][1].startswith("object 5: Illegal base64 character at index 0 of party 1's secretShares")
            assert parts[0] == parts[2] == (OK, "")
            check_against_oracle(cs, finish, res, bad_want=want)
        assert res[-2][5] == want[5] and np.array_equal(res[-2], ref[1][-2])
        for x, r in zip(res[:-3], ref[1][:-3]):  # every other object's bytes
            per = {1: cs.uoff, 16: cs.woff, 24: cs.woff}[1 if x.ndim == 1 else x.shape[1]]
            for o in range(cs.K):
                if o != 5:
                    lo = int(per[o])
                    hi = lo + cs.ulen[o] if x.ndim == 1 else int(per[o + 1])
                    assert np.array_equal(x[lo:hi], r[lo:hi]), o


# ---- illegal characters ----------------------------------------------------------------------------------
LIVE = [1, 2, 5, 7, 9]  # objects of 1, 192, 193, 385 and 191 words: field k's offender stands in LIVE[k]


def spoiled(L, cs, j, k_of, at_of, byte_of, residue):
    """Party j's bodies with one offender per object of k_of -- field k_of[o] at
    offset at_of[o] -- each body padded so that this field starts at `residue`
    mod 16; -> (bodies, starts, the same offenders as slotted buffers)."""
    _, base = bodies_for(L, cs, j)
    pads = {o: (residue - int(base[o, k])) % 16 for o, k in k_of.items()}
    bodies, starts = bodies_for(L, cs, j, pads=pads)
    bufs = cs.buffers()
    for o, k in k_of.items():
        assert int(starts[o, k]) % 16 == residue
        bodies[o][int(starts[o, k]) + at_of[o]] = byte_of[o]
        bufs[j][k][int(cs.foff[o]) + at_of[o]] = byte_of[o]
    return bodies, starts, bufs[j]


@pytest.mark.parametrize("residue", [0, 1, 15])
@pytest.mark.parametrize("where", ["first", "last"])
def test_an_illegal_character_at_each_end_of_each_field(A, ctx1, residue, where):
    L = A._lib
    cs = case("tiles", 3)
    k_of = {o: k for k, o in enumerate(LIVE)}
    at_of = {o: 0 if where == "first" else chars(cs.sizes[o]) - 1 for o in LIVE}
    byte_of = {o: ord("!") for o in LIVE}
    made = [bodies_for(L, cs, j) for j in range(3)]
    bodies, starts = [m[0] for m in made], [m[1] for m in made]
    bodies[1], starts[1], bufs1 = spoiled(L, cs, 1, k_of, at_of, byte_of, residue)
    bufs = cs.buffers()
    bufs[1] = bufs1
    want = {o: cs.bad_value(o, 1, k_of[o], at_of[o]) for o in LIVE}
    for finish in ("verify", "mask_json"):
        parts, res = run_bodies(ctx1, cs, bodies, starts, [2, 1, 0], finish)
        rparts, ref = run_session(ctx1, cs, bufs, [2, 1, 0], finish)
        assert {o: int(v) for o, v in enumerate(rparts[1][0]) if v >= 0} == want  # the slotted form's verdicts
        assert parts[1] == rparts[1][1] and parts[1][0] == E_PARAM and parts[0] == parts[2] == (OK, "")
        assert np.array_equal(res[-2], ref[-2]) and np.array_equal(res[-3], ref[-3]) and res[-1] == ref[-1]
        check_against_oracle(cs, finish, res, bad_want=want)


@pytest.mark.parametrize("i", range(len(TC.EDGE_BYTES)))
def test_the_edge_bytes(A, ctx1, i):
    """Each of TC's edge bytes in a fast tile (object 7, character 4,096 + 17)
    and in a last tile (object 5's last unit), field and residue rotating."""
    L = A._lib
    c = TC.EDGE_BYTES[i]
    cs = case("tiles", 1)
    k_of = {7: i % 5, 5: (i + 2) % 5}
    at_of = {7: 4096 + 17, 5: chars(193) - 7}
    bodies, starts, bufs0 = spoiled(L, cs, 0, k_of, at_of, {7: c, 5: c}, residue=(5 * i + 1) % 16)
    want = {o: cs.bad_value(o, 0, k_of[o], at_of[o]) for o in (5, 7)}
    parts, res = run_bodies(ctx1, cs, [bodies], [starts], [0], "verify")
    rparts, ref = run_session(ctx1, cs, [bufs0], [0], "verify")
    assert {o: int(v) for o, v in enumerate(rparts[0][0]) if v >= 0} == want
    assert parts[0] == rparts[0][1] and np.array_equal(res[-2], ref[-2]) and res[-1] == ref[-1]
    check_against_oracle(cs, "verify", res, bad_want=want)


# ---- hostile neighbours ------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", ["0xFF", "letters"])
def test_hostile_neighbours(A, ctx, fill):
    """Every byte of every body that is no text -- the JSON around the members,
    up to 15 of which share a granule with a text's first or last characters
    -- replaced by 0xFF, then by valid base64 letters: no output changes."""
    L = A._lib
    cs = case("tiles", 3)
    made = [bodies_for(L, cs, j, pad=6, tags="unicode") for j in range(3)]
    bodies, starts = [m[0] for m in made], [m[1] for m in made]
    for j in range(3):
        for o, W in enumerate(cs.sizes):
            raw = bodies[j][o]
            keep = np.zeros(len(raw), bool)
            for k in range(5):
                keep[int(starts[j][o, k]):int(starts[j][o, k]) + chars(W)] = True
            arr = np.frombuffer(bytes(raw), np.uint8).copy()
            other = np.full(len(raw), 0xFF, np.uint8) if fill == "0xFF" else \
                np.frombuffer((TC.ALPHABET * (len(raw) // 64 + 1))[:len(raw)], np.uint8)
            bodies[j][o] = bytearray(np.where(keep, arr, other).tobytes())
            assert len(bodies[j][o]) == len(raw)
    for finish in FINISHES:
        parts, res = run_bodies(ctx, cs, bodies, starts, [0, 2, 1], finish)
        assert all(parts[j] == (OK, "") for j in range(3))
        check_against_oracle(cs, finish, res)
        same(res, run_session(ctx, cs, cs.buffers(), [0, 2, 1], finish)[1])


# ---- modes and primes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("finish", FINISHES)
@pytest.mark.parametrize("shape", ["tiles", "forty"])
def test_device_mode_equals_host_mode(A, ctx1, shape, finish):
    L = A._lib
    cs = case(shape, 3, faults=((2, 3, 0),) if shape == "tiles" else ())
    made = [bodies_for(L, cs, j, pad=10, order=(3, 4, 0, 1, 2)) for j in range(3)]
    bodies, starts = [m[0] for m in made], [m[1].copy() for m in made]
    want = None
    if shape == "tiles":
        bodies[1][5][int(starts[1][5, 2]) + 17] = ord("!")
        starts[2][9] = ABSENT
        want = {5: cs.bad_value(5, 1, 2, 17), 9: 10 * chars(191)}
    _, hres = run_bodies(ctx1, cs, bodies, starts, [2, 0, 1], finish)
    _, dres = run_bodies(ctx1, cs, bodies, starts, [2, 0, 1], finish, dev=True)
    skip = set(want or ())
    rows = [o for o in range(cs.K) if o not in skip]
    assert np.array_equal(hres[-3][rows], dres[-3][rows]) and np.array_equal(hres[-2], dres[-2])
    check_against_oracle(cs, finish, hres, bad_want=want)
    dres = dres[:-3] + (np.where(dres[-2] >= 0, -1, dres[-3]), dres[-2], hres[-1])  # (device mode has no status)
    check_against_oracle(cs, finish, dres, bad_want=want)


def test_the_device_call_checks_its_arguments(A, ctx1):
    import torch
    L = A._lib
    cs = case("forty", 2)
    bodies, starts = bodies_for(L, cs, 0)
    at = np.concatenate([[0], np.cumsum([(len(b) + 15) & ~15 for b in bodies])]).astype(np.uint64)
    buf = np.zeros(int(at[-1]) + 16, np.uint8)
    for b, a in zip(bodies, at):
        buf[int(a):int(a) + len(b)] = np.frombuffer(bytes(b), np.uint8)
    dbuf = torch.from_numpy(buf).cuda()
    absolute = starts + at[:-1, None]
    with ctx1.clients_begin_dev(cs.woff, 2) as s:
        launches = ctx1.stats()["kernel_launches"]
        with pytest.raises(L.AmphoraNativeError, match="16") as e:  # a misaligned buffer
            s.party_bodies_dev(0, dbuf[1:], absolute)
        assert e.value.status == E_PARAM
        with pytest.raises(L.AmphoraNativeError, match="end past the") as e:
            s.party_bodies_dev(0, dbuf[:int(at[-1]) - 64], absolute)
        assert e.value.status == E_PARAM and s.parties_seen == 0 and ctx1.stats()["kernel_launches"] == launches
    with ctx1.clients_begin(cs.woff, 2) as s:
        with pytest.raises(ValueError):
            s.party_bodies_dev(0, dbuf, absolute)
        assert L.lib.amph_bodies_party_dev(s._h, 0, dbuf.data_ptr(), dbuf.numel(), absolute.ctypes.data, None) == E_PARAM
        assert "takes the host calls" in L.lib.amph_last_error().decode()


@pytest.mark.parametrize("pid", FC.PRIME_IDS)
def test_every_prime_both_modes(A, pid):
    """The any-alignment form in both prime regimes, on rows that reach a sum
    of exactly p, of p - 1 and (BIG) a carry out of bit 127 -- two objects that
    split the rows, against Python integers."""
    import torch
    L = A._lib
    pr = FC.BY_ID[pid]
    c = A.Context(pr.p, pr.r, pr.rinv)
    for n in (2, 3):
        rows = FC.odo_rows(pid, n)
        order = FC.session_orders(n)[-1]
        FC.assert_session_coverage(pr, rows, order)
        W = rows.W
        woff = np.asarray([0, W // 3, W], np.uint64)
        od = FC.odo_arrays(rows)
        want_sums = FC.running_sums(pr, rows, order)
        bodies, starts = [], []
        for j in range(n):
            bs, st = [], np.empty((2, 5), np.uint64)
            for o in range(2):
                a, b = int(woff[o]), int(woff[o + 1])
                raw = BC.body([b64(od[j][k][a:b]) for k in range(5)], order=(2, 0, 4, 1, 3), pad=3 + 5 * j + o).encode()
                st[o], _ = L.bodies_scan(raw)
                bs.append(raw)
            bodies.append(bs), starts.append(st)
        for dev in (False, True):
            s = c.clients_begin_dev(woff, n) if dev else c.clients_begin(woff, n)
            with s:
                for j in order:
                    s.party_bodies(j, bodies[j], starts[j])
                y, ff, bad = s.finish_verify()
                if dev:
                    torch.cuda.synchronize()
                    y, ff, bad = y.cpu().numpy(), ff.cpu().numpy(), bad.cpu().numpy()
                    ff, bad = np.where(ff == NF, -1, ff), np.where(bad == NF, -1, bad)
                assert (ff == -1).all() and (bad == -1).all(), (pid, n, dev, ff, bad)
                assert FC.ints(y) == list(rows.ys), (pid, n, dev)
                for o, i in ((0, 0), (1, 0), (1, W - W // 3 - 1)):
                    g = int(woff[o]) + i
                    assert s.word(o, i) == tuple(FC.from_gfp(pr, want_sums[k][g]) for k in range(5))


# ---- launches and copies -----------------------------------------------------------------------------------------
def test_launches_and_copies_do_not_depend_on_k(A, ctx):
    L = A._lib
    seen = {}
    for shape in ("one", "forty"):
        cs = case(shape, 3)
        made = [bodies_for(L, cs, j, pad=4) for j in range(3)]
        rows = []
        s = ctx.clients_begin(cs.woff, 3)
        for step in (0, 1, 2, "verify"):
            l0, c0, w0 = ctx.stats()["kernel_launches"], ctx.clients_copies(), ctx.wire_batch_copies()
            if step == "verify":
                s.finish_verify()
            else:
                s.party_bodies(step, [bytes(b) for b in made[step][0]], made[step][1])
            rows.append((ctx.stats()["kernel_launches"] - l0, ctx.clients_copies() - c0))
            assert ctx.wire_batch_copies() == w0
        s.close()
        seen[shape] = rows
    assert seen["one"] == seen["forty"]
    assert [x[0] for x in seen["one"]] == [1, 1, 1, 1]  # one launch per party call and one for the finish
    assert len({x[1] for x in seen["one"][:3]}) == 1 and seen["one"][0][1] in (0, 2)  # as amph_clients_party


def test_device_mode_launches_do_not_depend_on_k(A, ctx1):
    L = A._lib
    counts = []
    for shape in ("one", "forty"):
        cs = case(shape, 3)
        made = [bodies_for(L, cs, j) for j in range(3)]
        l0 = ctx1.stats()["kernel_launches"]
        with ctx1.clients_begin_dev(cs.woff, 3) as s:
            for j in range(3):
                s.party_bodies(j, [bytes(b) for b in made[j][0]], made[j][1])
            s.finish_verify()
        counts.append(ctx1.stats()["kernel_launches"] - l0)
    assert counts == [4, 4]


# ---- the Python layer -----------------------------------------------------------------------------------------------
def _outcomes_equal(got, want):
    assert len(got) == len(want)
    for o, (g, w) in enumerate(zip(got, want)):
        if isinstance(w, Exception):
            assert type(g) is type(w) and str(g) == str(w), (o, g, w)
        else:
            assert g == w, o


def _spy(monkeypatch, L):
    calls = {"party_bodies": 0, "party": 0}
    for name in calls:
        orig = getattr(L.ClientSessions, name)

        def wrapped(self, *a, _orig=orig, _name=name, **kw):
            calls[_name] += 1
            return _orig(self, *a, **kw)
        monkeypatch.setattr(L.ClientSessions, name, wrapped)
    return calls


def test_response_sessions_in_place_equals_the_gather(A, ctx1, monkeypatch):
    import uuid
    L, client = A._lib, A.client
    util = client.SecretShareUtil(ctx1)
    cs = Case([3, 193, 2, 1, 5], 3, seed=900, faults=((2, 3, 1),))
    sids = [uuid.UUID(int=o + 1) for o in range(cs.K)]

    def make(j, o, texts=None, **kw):
        return BC.body(texts or [b64(f) for f in cs.objs[o][j]], sid=str(sids[o]), pad=(3 * o + j) % 16, **kw)
    bodies = [[make(j, o, tags=("plain", "unicode", "quotes")[j]) for o in range(cs.K)] for j in range(3)]
    spoiled_ = [b64(f) for f in cs.objs[3][1]]
    spoiled_[2] = b"!" + spoiled_[2][1:]          # object 3: an illegal character
    bodies[1][3] = make(1, 3, spoiled_)
    short = [b64(f) for f in cs.objs[4][2]]
    short[3] = short[3][:-4]                      # object 4: one member a group short
    bodies[2][4] = make(2, 4, short)
    calls = _spy(monkeypatch, L)
    results = {}
    for in_place in (True, False):
        with client.ResponseSessions(util, 3, in_place=in_place) as rs:
            for j in (2, 0, 1):
                rs.add_bodies(j, bodies[j])
            results[in_place] = rs.secrets(sids)
    assert calls == {"party_bodies": 3, "party": 3}
    _outcomes_equal(results[True], results[False])
    lists = [[bodies[j][o] for j in range(3)] for o in range(cs.K)]
    want = client.verify_vss_json_batch(util, lists, sids)
    for o in (0, 1, 2, 3):  # (object 4's ragged member: the sessions' own message, equal in both forms above)
        _outcomes_equal([results[True][o]], [want[o]])
    assert isinstance(results[True][2], A.IntegrityVerificationException)
    assert isinstance(results[True][3], A.AmphoraClientException) and isinstance(results[True][4], A.AmphoraClientException)
    assert results[True][1][2] == FC.ints(cs.y[1])
    # the first party's bodies fix the word table: a first body that is not whole words fails its secret alone
    odd = [list(b) for b in bodies]
    odd[2][0] = make(2, 0, [t[:-4] for t in [b64(f) for f in cs.objs[0][2]]])
    for in_place in (True, False):
        with client.ResponseSessions(util, 3, in_place=in_place) as rs:
            for j in (2, 0, 1):
                rs.add_bodies(j, odd[j])
            results[in_place] = rs.secrets(sids)
    _outcomes_equal(results[True], results[False])
    assert isinstance(results[True][0], A.AmphoraClientException) and results[True][1][2] == FC.ints(cs.y[1])


def test_a_body_with_an_escaped_member_takes_the_fallback(A, ctx1, monkeypatch):
    import uuid
    L, client = A._lib, A.client
    util = client.SecretShareUtil(ctx1)
    cs = Case([3, 2], 2, seed=950)
    sids = [uuid.UUID(int=o + 1) for o in range(cs.K)]
    bodies = [[BC.body([b64(f) for f in cs.objs[o][j]], sid=str(sids[o]), pad=j + o) for o in range(cs.K)]
              for j in range(2)]
    t = [b64(f).decode() for f in cs.objs[1][1]]
    assert "/" in t[0] + t[1] + t[2] + t[3] + t[4]
    k = [i for i in range(5) if "/" in t[i]][0]
    t[k] = t[k].replace("/", "\\/", 1)  # a legal JSON escape: not the plain form
    bodies[1][1] = BC.body(t, sid=str(sids[1]), pad=2)
    with pytest.raises(L.BodyNotPlain, match="backslash"):
        L.bodies_scan(bodies[1][1].encode())
    calls = _spy(monkeypatch, L)
    results = {}
    for in_place in (True, False):
        with client.ResponseSessions(util, 2, in_place=in_place) as rs:
            rs.add_bodies(0, bodies[0])
            rs.add_bodies(1, bodies[1])
            results[in_place] = rs.secrets(sids)
    assert calls == {"party_bodies": 1, "party": 3}  # party 1's call of the in-place session went the old way
    _outcomes_equal(results[True], results[False])
    assert results[True][0][2] == FC.ints(cs.y[0]) and isinstance(results[True][1], A.AmphoraClientException)
    # a null member: the reference's exception, raised by add_bodies itself, in both forms
    nulled = bodies[0][0].replace('"vShares":"%s"' % b64(cs.objs[0][0][2]).decode(), '"vShares":null')
    for in_place in (True, False):
        with client.ResponseSessions(util, 2, in_place=in_place) as rs:
            with pytest.raises(A.IllegalArgumentException, match="vShares is marked non-null but is null"):
                rs.add_bodies(0, [nulled, bodies[0][1]])
