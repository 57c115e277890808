"""The verdict catalogue (tests/verdict_cases.py) on the CPU: its self-check
for every prime, party count and size tests/test_hip_verdicts.py uses, the C
oracle and the Python restatement of the reference client against the plain
Python-int verdicts -- the oracle's own ``u == v r`` half was pinned by nothing
before -- and the library's host-side failure message for a fault in one half
of the predicate only."""
import functools

import pytest

from oracle import amphora_oracle as O
from oracle import coracle
from tests import field_cases as FC
from tests import verdict_cases as VC

PRIMES = ["test", "m89"]
SIZES = [(1217, "ABCDE"), (257, "ABCDE"), (192, "A"), (1, "A")]


@functools.lru_cache(maxsize=None)
def _field(pid):
    pr = FC.BY_ID[pid]
    return coracle.Field(pr.p, pr.r, pr.rinv, threads=4)


@pytest.mark.parametrize("n", FC.PARTY_COUNTS)
@pytest.mark.parametrize("pid", PRIMES)
def test_catalogue_self_check(pid, n):
    pr = FC.BY_ID[pid]
    for W, classes in SIZES:
        b, cs = VC.catalogue(pid, n, W, classes)  # runs VC.self_check: every reference verdict is the declared one
        seen = VC.self_check(b, [c for c, _ in cs])
        assert set(seen) == set(classes) and all(seen[k] >= 1 for k in classes), (W, seen)
        a_fields = {VC.FIELDS[c.edits[0][1]] for c, _ in cs if c.cls == "A"}
        assert a_fields == set(VC.FIELDS), (W, a_fields)
        names = [c.name for c, _ in cs]
        assert len(names) == len(set(names))
        if W >= 192:  # every limb of the compare a prime of that size has: one bit of it, nothing else
            limbs = {k: {c.limb for c, _ in cs if c.cls == "A" and c.edits[0][1] == k} - {None} for k in (VC.Wf, VC.U)}
            want = {q for q in range(4) if (1 << 32 * q) < pr.p and (q < 3 or pr.big)}
            assert limbs[VC.Wf] == limbs[VC.U] == want, (W, limbs)
        if "B" in classes:
            assert sum(x.endswith("_plus_p") for x in names) == 5
            assert sum(x.endswith("_plus_kp") for x in names) == (5 if pid == "m89" else 0)  # the largest k that fits
            assert sum(x.endswith("_cancel") for x in names) == (2 if n >= 2 else 0)
        if "E" in classes:
            assert ("E_1023v_1024u" in names) == (W > 1024) and "E_191u_192w" in names
        # accepted cases leave the secrets alone except the one that is built to change them
        for c, e in cs:
            if e.ff < 0:
                assert bool(e.changed) == (c.name == "D_y_with_w"), c.name


@pytest.mark.parametrize("n", FC.PARTY_COUNTS)
@pytest.mark.parametrize("pid", PRIMES)
def test_c_oracle_agrees_on_every_case(pid, n):
    """orc_recombine_verify / orc_mask_input on the edited arrays: secrets,
    masked words and first-fail are the Python-int reference's."""
    pr, F = FC.BY_ID[pid], _field(pid)
    for W, classes in SIZES[:2]:
        b, cs = VC.catalogue(pid, n, W, classes)
        arrays = VC.base_arrays(b)
        secrets = VC.secrets_for(b)
        sec = FC.arr(secrets)
        y, ff = F.recombine_verify(arrays)
        assert ff == -1 and FC.ints(y) == list(b.cols[VC.Y])
        for c, e in cs:
            bad, _ = VC.apply(arrays, c)
            ys = VC.patched(b.cols[VC.Y], e.changed)
            y, ff = F.recombine_verify(bad)
            assert ff == e.ff and FC.ints(y) == ys, (W, c.name, ff, e.ff)
            m, ff = F.mask_input(sec, bad)
            assert ff == e.ff and FC.ints(m) == FC.mask_words(pr, secrets, ys), (W, c.name, ff, e.ff)


@pytest.mark.parametrize("n", [1, 3])
def test_python_restatement_of_the_client_on_one_fault_per_field(n):
    """oracle.amphora_oracle.verify_output_delivery_objects (the BigInteger
    restatement) on a 64-word base: one A case per field."""
    pr = FC.BY_ID["test"]
    b, cs = VC.catalogue("test", n, 64)
    util = O.ClientSecretShareUtil(pr.p, pr.r, pr.rinv)
    arrays = VC.base_arrays(b)
    objects = lambda arrs: [O.OutputDeliveryObject(*[f.tobytes() for f in o]) for o in arrs]  # noqa: E731
    assert O.verify_output_delivery_objects(util, objects(arrays)) == list(b.cols[VC.Y])
    picked = [c for c, _ in cs if c.name.endswith("_plus1")]
    assert [VC.FIELDS[c.edits[0][1]] for c in picked] == list(VC.FIELDS)
    for c in picked:
        e = VC.expect(b, c)
        y, r, v, w, u = VC.columns(b, c)
        with pytest.raises(O.IntegrityVerificationException) as err:
            O.verify_output_delivery_objects(util, objects(VC.apply(arrays, c)[0]))
        assert str(err.value) == O.verification_failure_message(pr.p, e.ff, y, r, u, v, w), c.name
    for c, e in cs:
        if e.ff < 0:
            assert O.verify_output_delivery_objects(util, objects(VC.apply(arrays, c)[0])) == \
                VC.patched(b.cols[VC.Y], e.changed), c.name


def _halves(message):
    """The last line "\\t{w} = {y r}   &&   {u} = {v r}" as ((w, y r), (u, v r))."""
    w_half, u_half = message.split("\n")[-1].strip().split("   &&   ")
    return tuple(tuple(int(x) for x in h.split(" = ")) for h in (w_half, u_half))


@pytest.mark.parametrize("pid", PRIMES)
def test_failure_message_names_the_half_that_failed(pid):
    """amph_verify_message runs on the host: for a u-only fault the w half
    shows equal sides and the u half unequal ones, and the other way round."""
    import amphora_amd
    pr = FC.BY_ID[pid]
    ctx = amphora_amd.Context(pr.p, pr.r, pr.rinv)
    b, cs = VC.catalogue(pid, 2, 64)
    by_name = {c.name: (c, e) for c, e in cs}
    for name, broken in (("A_u_plus1", 1), ("A_w_plus1", 0)):
        c, e = by_name[name]
        y, r, v, w, u = (col[e.ff] for col in VC.columns(b, c))
        msg = ctx.verify_message(y, r, u, v, w)
        assert msg == O.verification_failure_message(pr.p, 0, [y], [r], [u], [v], [w])
        halves = _halves(msg)
        assert halves[0] == (w, y * r % pr.p) and halves[1] == (u, v * r % pr.p)
        assert (halves[broken][0] != halves[broken][1]) and (halves[1 - broken][0] == halves[1 - broken][1]), name
