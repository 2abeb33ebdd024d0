"""The per-read text kernels past their grid cap.  Eight launches run "one wave per record,
grid-stride" on at most 65,536 workgroups of four waves, so beyond CAP = 262,144 records every
wave takes a second trip round its loop; the rest of the suite stays at or below CAP in all of
them but k_fasta<false>.  The batches of grid_cap_lib.py hold CAP + 5 records (test_grid_cap.py
pins them on the host), and each test below names the launch it drives past the cap.

Every comparison is byte or array equality against the host parser, the host-parsed encode, or
the plain Python models (names_lib, qual_lib, pair_lib, range_lib)."""
import ctypes
import functools

import numpy as np
import pytest

import grid_cap_lib as gc
import names_lib as nl
import ntcomp_amd as nt
import pair_lib as pl
import qual_lib as ql
import range_lib as rl
from grid_cap_lib import CAP, N, N_PAIRS
from test_grid_cap import host_parse, long_read, parse_shapes

pytestmark = pytest.mark.gpu
FORMAT = 8
BR = 65536  # the default block: four whole sections and one of five reads
FORMS = ["fasta", "fastq", "named_fasta", "named_fastq"]


@pytest.fixture(scope="module")
def ctx():
    genome = nt.synth_genome(7, 20_000)
    c = nt.GpuContext(0)
    c.upload(nt.Index.build([genome.tobytes()], 31))
    yield c
    c.close()


@pytest.fixture()
def paired(ctx):
    ctx.paired = "ids"
    yield ctx
    ctx.paired = "off"


def _blob(metas):
    return b"".join(ctypes.string_at(ctypes.byref(m), ctypes.sizeof(m)) for m in metas)


def _flat(out):
    """an encode call's result with quality and name sections, as comparable bytes"""
    metas, payload, nb, (qm, qp), (nm, npay) = out
    return (_blob(metas), payload, nb, _blob(qm), qp, _blob(nm), npay)


def _unpack(ctx, metas, payload, n):
    arr = (nt.BlockMeta * len(metas))(*metas)
    assert ctx.unpack(arr, payload, len(metas))[:2] == (len(metas), n)


def _fasta(reads, first_id=1):
    return b"".join(b">seq.%d\n%s\n" % (first_id + i, r) for i, r in enumerate(reads))


_SCRUB = b"@scrubbed\nACGTACGT\n+\nIIIIIIII\n"


@functools.lru_cache(maxsize=None)
def _scrub_text(n):
    return _SCRUB * n


def _scrub(ctx, n, at_least=0):
    """A context keeps its workspaces from call to call, so a kernel that skipped its second trip
    would go unnoticed wherever the call before left the same bytes (the raw text, kept counts,
    offsets, bases, qualities, the names' columns).  Before a call whose result is compared, this
    takes n records that differ from the batch's in every one of those, in at least as many bytes
    of text, through the same workspaces."""
    text = _scrub_text(n)
    assert len(text) >= at_least
    ctx.encode_pack_fastq(text, n, qualities="keep", names="keep")


def _assert_same(got, want):
    """equality, with the first differing byte named where it fails (not two 4 MB reprs)"""
    if got != want:
        a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
        k = min(len(a), len(b))
        d = np.flatnonzero(a[:k] != b[:k])
        at = int(d[0]) if len(d) else k
        raise AssertionError(f"{len(got)} bytes for {len(want)}; first difference at byte {at}: "
                             f"{got[max(0, at - 20):at + 20]!r} for {want[max(0, at - 20):at + 20]!r}")


def _assert_bases(got, want, offs):
    """equality of parsed bases, with the record of the first differing base where it fails"""
    if not np.array_equal(got, want):
        k = min(len(got), len(want))
        d = np.flatnonzero(got[:k] != want[:k])
        at = int(d[0]) if len(d) else k
        raise AssertionError(f"{len(got)} bases for {len(want)}; first difference at base {at}, "
                             f"record {int(np.searchsorted(offs, at, side='right')) - 1}")


@pytest.fixture(scope="module")
def plain():
    """the batch, its records one by one and its LF text"""
    names, reads, quals = gc.batch(long_read=long_read())
    recs = gc.records(names, reads, quals)
    return dict(names=names, reads=reads, quals=quals, recs=recs, text=b"".join(recs))


@pytest.fixture(scope="module")
def parsed(plain, tmp_path_factory):
    """{shape: (text, the host parser's bases, its offsets)}"""
    d = tmp_path_factory.mktemp("grid_cap")
    out = {}
    for shape, (text, _) in parse_shapes(plain["names"], plain["reads"], plain["quals"]).items():
        (d / "x.fq").write_bytes(text)
        out[shape] = (text, *host_parse(d / "x.fq"))
    assert out["lf"][0] == plain["text"]
    return out


# ---- parse ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["lf", "crlf_messy", "no_last_newline"])
def test_parse_equals_the_host_parser(ctx, parsed, shape):
    """launch_fastq_parse: k_fq_recs (kept counts, the structure checks) and k_fq_norm (the bases)
    over CAP + 5 records; crlf_messy has IUPAC symbols, lower case and blanks on the second trip"""
    text, bases, offs = parsed[shape]
    _scrub(ctx, N, len(text))
    gb, go = ctx.parse_fastq(text, N)
    assert np.array_equal(go, offs)
    _assert_bases(gb, bases, offs)


@pytest.mark.parametrize("n", [CAP, CAP + 1])
def test_parse_at_the_last_size_with_one_trip_and_the_first_with_two(ctx, plain, parsed, n):
    """launch_fastq_parse (k_fq_recs, k_fq_norm) on prefixes of the LF text: a full grid and one
    trip, then one wave with a second trip"""
    _, bases, offs = parsed["lf"]
    _scrub(ctx, N, len(plain["text"]))  # (the full text went through before: kept[CAP] and its bases would be there)
    gb, go = ctx.parse_fastq(b"".join(plain["recs"][:n]), n)
    assert np.array_equal(go, offs[:n + 1])
    _assert_bases(gb, bases[:int(offs[n])], offs)


def _record(plain, i, name=None, qual=None, plus=b"+"):
    name = b"@" + plain["names"][i] if name is None else name
    return name + b"\n" + plain["reads"][i] + b"\n" + plus + b"\n" + (plain["quals"][i] if qual is None else qual) + b"\n"


def test_parse_errors_beyond_the_cap_name_their_record(ctx, plain, parsed):
    """k_fq_recs reports from a second-trip wave with that trip's record number (fq_fail), and the
    lowest bad record wins across the trips"""
    header = _record(plain, CAP + 2, name=b">" + plain["names"][CAP + 2])
    cases = {"header": ({CAP + 2: header}, CAP + 2),
             "plus": ({CAP + 3: _record(plain, CAP + 3, plus=b"-")}, CAP + 3),
             "qual_short": ({N - 1: _record(plain, N - 1, qual=plain["quals"][N - 1][:-1])}, N - 1),
             "two": ({1000: _record(plain, 1000, plus=b"-"), CAP + 2: header}, 1000)}
    for name, (changes, bad) in cases.items():
        with pytest.raises(nt.NtcError) as e:
            ctx.parse_fastq(gc.swap(plain["recs"], changes), N)
        assert e.value.code == FORMAT and e.value.bad_read == bad, (name, e.value.bad_read)
    _, bases, offs = parsed["lf"]
    _scrub(ctx, N, len(plain["text"]))  # (a failed parse writes no base: the last sound one's would still be there)
    gb, go = ctx.parse_fastq(plain["text"], N)  # no status word is carried over
    assert np.array_equal(go, offs)
    _assert_bases(gb, bases, offs)


# ---- encode with the side sections ------------------------------------------------------------------
@pytest.fixture(scope="module")
def encoded(ctx, plain):
    _scrub(ctx, N, len(plain["text"]))
    return ctx.encode_pack_fastq(plain["text"], N, qualities="keep", names="keep")


@pytest.fixture(scope="module")
def qual_sections(plain):
    return ql.sections(plain["text"], BR)


@pytest.fixture(scope="module")
def name_sections(plain):
    return nl.sections(plain["names"], BR)


def _check_quals(got, want):
    qm, qp = got
    assert [ql.meta_dict(m) for m in qm] == want[0]
    assert np.array_equal(np.frombuffer(qp, dtype="<u8"), want[1])


def test_encode_keeps_names_and_qualities(ctx, parsed, encoded, name_sections, qual_sections):
    """launch_names_pack: k_n_measure over CAP + 5 records, behind launch_fastq_parse (k_fq_recs,
    k_fq_norm); k_q_gather rides along"""
    metas, payload, nb, quals, (nm, npay) = encoded
    _, bases, offs = parsed["lf"]
    m0, p0 = ctx.encode_pack(bases, offs)
    assert nb == len(bases) and len(metas) == 5 and all(m.status == 0 and m.num_records for m in metas)  # no block dropped
    assert _blob(metas) == _blob(m0) and payload == p0
    assert [nl.meta_dict(m) for m in nm] == name_sections[0]
    _assert_same(npay, name_sections[1])
    _check_quals(quals, qual_sections)


def test_encode_cuts_names_at_blanks_beyond_the_cap(ctx, plain, encoded, name_sections, qual_sections):
    """launch_names_pack: k_n_measure in mode id, the cut (ballot + ctz) taken on the second trip"""
    names, reads, quals = gc.batch(blanks=True, long_read=long_read())
    assert reads == plain["reads"] and quals == plain["quals"] and names[CAP:] != plain["names"][CAP:]
    text = nl.make_fastq(names, reads, quals)
    _scrub(ctx, N, len(text))  # (the sections are the plain batch's: its encode must not have left them)
    metas, payload, nb, qs, (nm, npay) = ctx.encode_pack_fastq(text, N, qualities="keep", names="id")
    assert (_blob(metas), payload, nb) == (_blob(encoded[0]), encoded[1], encoded[2])
    assert [nl.name_of(b"@" + n, "id") for n in names] == plain["names"]  # so the sections are the plain batch's
    assert [nl.meta_dict(m) for m in nm] == name_sections[0]
    _assert_same(npay, name_sections[1])
    _check_quals(qs, qual_sections)


def test_encode_errors_beyond_the_cap_name_their_record(ctx, plain, encoded):
    """k_n_measure (a name past 4,095 bytes) and k_q_gather (a byte outside '!'..'~') report the
    second trip's record number"""
    cases = {"name": {CAP + 3: _record(plain, CAP + 3, name=b"@" + b"n" * 4096)},
             "quality": {CAP + 4: _record(plain, CAP + 4, qual=b"\x1f" + plain["quals"][CAP + 4][1:])}}
    for name, changes in cases.items():
        (bad,) = changes
        with pytest.raises(nt.NtcError) as e:
            ctx.encode_pack_fastq(gc.swap(plain["recs"], changes), N, qualities="keep", names="keep")
        assert e.value.code == FORMAT and e.value.bad_read == bad, (name, e.value.bad_read)
    _scrub(ctx, N, len(plain["text"]))
    again = ctx.encode_pack_fastq(plain["text"], N, qualities="keep", names="keep")
    assert _flat(again) == _flat(encoded)


# ---- the formatters ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def whole(plain):
    """the text of every form, from the models; first_id 1 crosses every digit count from 1 to 6"""
    names, reads, quals = plain["names"], plain["reads"], plain["quals"]
    t = {"fasta": _fasta(reads), "fastq": ql.fastq_text(list(zip(reads, quals))),
         "named_fasta": nl.named_text(names, reads), "named_fastq": nl.named_text(names, reads, quals)}
    assert t["named_fastq"] == plain["text"] and b">seq.%d\n" % N in t["fasta"]
    return t


def _decode(ctx, encoded, form, window=None, first_id=1, n=N):
    """one batch through ntc_decode_fasta_unpacked in form, in test_gpu_names.py's order of calls"""
    metas, payload, _, (qm, qp), (nm, npay) = encoded
    _unpack(ctx, metas, payload, n)
    if form.startswith("named"):
        ctx.set_names(nm, npay)
    if form.endswith("fastq"):
        ctx.set_qualities(qm, qp)
    if window is not None:
        ctx.set_window(*window)
    return ctx.decode_fasta_unpacked(first_id=first_id)


@pytest.mark.parametrize("form", FORMS)
def test_text_of_every_form(ctx, encoded, whole, form):
    """launch_fasta k_fasta<false> (fasta), launch_fastq_text k_fastq<false> (fastq),
    launch_named_text k_named<false> with and without qualities (named_fasta, named_fastq)"""
    _assert_same(_decode(ctx, encoded, form), whole[form])


@pytest.mark.parametrize("form", FORMS)
def test_a_window_across_the_cap_and_one_beyond_it(ctx, encoded, whole, form):
    """the W = true instantiations and w_skips: launch_fasta k_fasta<true>, launch_fastq_text
    k_fastq<true>, launch_named_text k_named<true> (both forms); the reads keep their own ids,
    names and qualities"""
    for first, count in [(CAP - 2, 5), (CAP + 1, 3)]:
        got = _decode(ctx, encoded, form, (first, count))
        assert got == rl.cut(whole[form], first, first + count), (first, count)
    _assert_same(_decode(ctx, encoded, form), whole[form])  # and the window is gone


# ---- pairs ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mates(ctx):
    """N_PAIRS pairs: the sides, their texts, the woven text and its encode under paired = ids"""
    s1, s2 = gc.pairs(long_read=long_read())
    t1, t2 = nl.make_fastq(*s1), nl.make_fastq(*s2)
    woven = pl.weave(t1, t2)
    ctx.paired = "ids"
    try:
        _scrub(ctx, 2 * N_PAIRS, len(woven))
        ref = ctx.encode_pack_fastq(woven, 2 * N_PAIRS, qualities="keep", names="keep")
    finally:
        ctx.paired = "off"
    return dict(s1=s1, s2=s2, t1=t1, t2=t2, woven=woven, ref=ref, recs2=gc.records(*s2))


@pytest.mark.parametrize("shape", ["lf", "no_nl_1", "no_nl_2"])
def test_weave_equals_the_interleaved_call(paired, mates, shape):
    """launch_pair_weave: k_pw_copy over CAP + 5 pairs, and launch_pair_check: k_pm_check passing
    both strip rules on its second trip; the last pair (a second-trip wave's) adds the newline a
    text lacks"""
    t1 = mates["t1"][:-1] if shape == "no_nl_1" else mates["t1"]
    t2 = mates["t2"][:-1] if shape == "no_nl_2" else mates["t2"]
    # k_pw_copy writes where the reference call's woven text lay: it must find another text there,
    # and no newline where the last pair adds one
    woven = mates["woven"]
    _scrub(paired, 2 * N_PAIRS, len(woven))
    for at in (len(woven) - 1, len(woven) - 1 - len(mates["recs2"][-1])):
        assert woven[at:at + 1] == b"\n" != _scrub_text(2 * N_PAIRS)[at:at + 1]
    got = paired.encode_pack_fastq_paired(t1, t2, N_PAIRS, qualities="keep", names="keep")
    assert _flat(got) == _flat(mates["ref"])
    assert got[2] == sum(len(r) for r in mates["s1"][1] + mates["s2"][1])


def test_mates_that_disagree_beyond_the_cap(paired, mates):
    """launch_pair_check: k_pm_check reports pair CAP + 1 as read 2 (CAP + 1) from its second
    trip, and a lower bad pair wins across the trips"""
    n1, n2, recs2 = mates["s1"][0], mates["s2"][0], mates["recs2"]
    spoil = lambda p: b"@" + n2[p][:1] + b"#" + n2[p][1:] + recs2[p][1 + len(n2[p]):]
    for bad in [(CAP + 1,), (CAP + 1, 77), (CAP + 2, CAP + 4)]:  # (CAP + 1: "x<i>\t2:N", CAP + 2: "x<i>/2")
        # (the batch's own mates agree, test_grid_cap.py: the lowest spoiled pair is the first bad one)
        assert all(not pl.mates_agree(n1[p], n2[p][:1] + b"#" + n2[p][1:]) for p in bad)
        with pytest.raises(nt.NtcError) as e:
            paired.encode_pack_fastq_paired(mates["t1"], gc.swap(recs2, {p: spoil(p) for p in bad}), N_PAIRS,
                                            qualities="keep", names="keep")
        assert e.value.code == FORMAT and e.value.bad_read == 2 * min(bad) and "mates" in str(e.value), bad
    _scrub(paired, 2 * N_PAIRS, len(mates["woven"]))
    got = paired.encode_pack_fastq_paired(mates["t1"], mates["t2"], N_PAIRS, qualities="keep", names="keep")
    assert _flat(got) == _flat(mates["ref"])  # no status word is carried over


@pytest.fixture(scope="module")
def split_models(mates):
    """{form: (lines per record, the two parts of the whole text, its records)}, from the models"""
    reads = [r for two in zip(mates["s1"][1], mates["s2"][1]) for r in two]
    out = {}
    for form, lines, model in (("fasta", 2, _fasta(reads)), ("named_fastq", 4, mates["woven"])):
        out[form] = (lines, pl.split(model, lines), rl.records(model))  # (records: range_lib.cut's own first step)
    return out


@pytest.mark.parametrize("form", ["fasta", "named_fastq"])
def test_split_of_the_decoded_text(paired, mates, split_models, form):
    """launch_pair_split: k_ps_copy over 2 (CAP + 5) reads, three trips, behind launch_fasta
    k_fasta (fasta) or launch_named_text k_named (named_fastq); then windows of whole pairs
    across read CAP and read 2 CAP, where its trips change"""
    lines, want, recs = split_models[form]
    got = _decode(paired, mates["ref"], form, n=2 * N_PAIRS)
    _assert_same(got[0], want[0])
    _assert_same(got[1], want[1])
    assert paired.pair_split() == len(want[0])
    if form == "named_fastq":
        assert got == (mates["t1"], mates["t2"])
    for first, count in [(CAP - 2, 4), (2 * CAP - 2, 6)]:
        got = _decode(paired, mates["ref"], form, (first, count), n=2 * N_PAIRS)
        assert got == pl.split(b"".join(recs[first:first + count]), lines), (first, count)


# ---- id width ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("first_id", [4_294_967_290, 9_999_999_990, 18_446_744_073_709_551_000])
def test_ids_past_32_bits_and_up_to_twenty_digits(ctx, first_id):
    """k_fasta_sizes / k_fasta and k_fastq_sizes / k_fastq each carry their own digit code: ids
    across 2^32, from 10 to 11 digits, and of 20 digits, against Python's %d; named text has no id"""
    names, reads, quals = gc.batch(5, 40, long_read=long_read())
    enc = ctx.encode_pack_fastq(nl.make_fastq(names, reads, quals), 40, qualities="keep", names="keep")
    assert len(str(first_id)) in (10, 20) and first_id + 39 < 1 << 64
    assert len({len(str(first_id + i)) for i in range(40)}) == (2 if first_id == 9_999_999_990 else 1)
    assert _decode(ctx, enc, "fasta", first_id=first_id, n=40) == _fasta(reads, first_id)
    assert _decode(ctx, enc, "fastq", first_id=first_id, n=40) == ql.fastq_text(list(zip(reads, quals)), first_id)
    assert _decode(ctx, enc, "named_fasta", first_id=first_id, n=40) == nl.named_text(names, reads)
    assert _decode(ctx, enc, "named_fastq", first_id=first_id, n=40) == nl.named_text(names, reads, quals)
    assert _decode(ctx, enc, "fasta", (38, 2), first_id=first_id, n=40) == rl.cut(_fasta(reads, first_id), 38, 40)
