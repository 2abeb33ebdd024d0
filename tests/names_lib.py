"""Read names, restated in plain Python / numpy, independent of the library: the name of a
header line per mode, the canonical section of a block (include/ntcomp_codec.h "FASTQ read
names"), the expander, and a FASTQ maker with names.  The tests compare the GPU's and the
side file's bytes with these exactly: the form is unique."""
import struct

import numpy as np

MODES = {"drop": 0, "keep": 1, "id": 2}
NAME_MAX, GROUP, CAP = 4095, 64, 255


def name_of(header, mode="keep"):
    """header: the header line without its newline (b"@..." possibly ending in "\\r")."""
    assert header[:1] == b"@"
    n = header[1:]
    if n.endswith(b"\r"):
        n = n[:-1]
    if mode == "id":
        for i, c in enumerate(n):
            if c in b" \t":
                return n[:i]
    return n


def names_of(text, mode="keep"):
    """the names of FASTQ text made of whole four-line records (the last newline may lack)"""
    lines = text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    assert len(lines) % 4 == 0
    return [name_of(h, mode) for h in lines[0::4]]


def _lcp(a, b):
    n = min(len(a), len(b))
    if a[:n] == b[:n]:
        return n
    x = int.from_bytes(a[:n], "big") ^ int.from_bytes(b[:n], "big")  # the first byte that differs, from the top
    return n - (x.bit_length() + 7) // 8


def columns(names):
    """(len, pre, suf, mids) of one block's names"""
    lens, pres, sufs, mids = [], [], [], []
    for i, n in enumerate(names):
        assert len(n) <= NAME_MAX and b"\n" not in n
        pre = suf = 0
        if i % GROUP:
            p = names[i - 1]
            pre = min(CAP, _lcp(p, n))
            suf = min(CAP, _lcp(p[::-1], n[::-1]), len(p) - pre, len(n) - pre)
        lens.append(len(n))
        pres.append(pre)
        sufs.append(suf)
        mids.append(n[pre:len(n) - suf])
    return lens, pres, sufs, mids


def section(names):
    """-> (meta dict without payload_off, payload bytes)"""
    lens, pres, sufs, mids = columns(names)
    mid = b"".join(mids)
    body = np.array(lens, dtype="<u2").tobytes() + bytes(pres) + bytes(sufs) + mid
    body += bytes(-len(body) % 8)
    return dict(n_reads=len(names), name_bytes=sum(lens), mid_bytes=len(mid), payload_bytes=len(body)), body


def sections(names, block_reads):
    """every block of block_reads names -> (list of meta dicts with payload_off, payload bytes)"""
    metas, pay = [], b""
    for a in range(0, len(names), block_reads):
        m, body = section(names[a:a + block_reads])
        m["payload_off"] = len(pay)
        metas.append(m)
        pay += body
    return metas, pay


def expand(meta, body):
    """a section back to its names; ValueError where the rules of the format are broken"""
    n = meta["n_reads"]
    if meta["payload_bytes"] != (4 * n + meta["mid_bytes"] + 7) // 8 * 8 or len(body) != meta["payload_bytes"]:
        raise ValueError("payload size")
    lens = np.frombuffer(body, dtype="<u2", count=n).tolist()
    pres, sufs = list(body[2 * n:3 * n]), list(body[3 * n:4 * n])
    at, names, prev = 4 * n, [], b""
    for i in range(n):
        ln, pre, suf = lens[i], pres[i], sufs[i]
        if ln > NAME_MAX:
            raise ValueError("len")
        if i % GROUP == 0:
            if pre or suf:
                raise ValueError("restart")
        elif pre + suf > min(ln, len(prev)):
            raise ValueError("pre + suf")
        m = ln - pre - suf
        if at + m > 4 * n + meta["mid_bytes"]:
            raise ValueError("mids")
        names.append(prev[:pre] + body[at:at + m] + prev[len(prev) - suf:])
        at += m
        prev = names[-1]
    if at != 4 * n + meta["mid_bytes"] or sum(lens) != meta["name_bytes"] or any(body[at:]):
        raise ValueError("sums or padding")
    return names


def meta_dict(m):
    """a NameMeta (or anything with its fields) as the dict sections() makes"""
    return {k: int(getattr(m, k)) for k in ("n_reads", "name_bytes", "mid_bytes", "payload_bytes", "payload_off")}


def make_fastq(names, reads, quals=None, eol=b"\n", last_newline=True):
    out = []
    for i, (n, r) in enumerate(zip(names, reads)):
        q = quals[i] if quals is not None else b"I" * len(r)
        out.append(b"@" + n + eol + r + eol + b"+" + eol + q + eol)
    text = b"".join(out)
    return text if last_newline or not text else text[:-len(eol)]


def named_text(names, reads, quals=None):
    """what decode prints with name sections pending (and quality sections, when quals)"""
    if quals is None:
        return b"".join(b">" + n + b"\n" + r + b"\n" for n, r in zip(names, reads))
    return b"".join(b"@" + n + b"\n" + r + b"\n+\n" + q + b"\n" for n, r, q in zip(names, reads, quals))


def illumina_names(rng, n, comment=True):
    """A00123:45:HXXXXDSXX:1:1101:x:y 1:N:0:ATCACGTT+AGGCTATA with x ascending, y random"""
    out, x = [], 1000
    for _ in range(n):
        x += int(rng.integers(0, 30))
        s = b"A00123:45:HXXXXDSXX:1:1101:%d:%d" % (x, int(rng.integers(1000, 40000)))
        out.append(s + (b" 1:N:0:ATCACGTT+AGGCTATA" if comment else b""))
    return out


def sra_names(n, length=150):
    return [b"SRR1234567.%d %d length=%d" % (i + 1, i + 1, length) for i in range(n)]


def edge_names():
    """lengths 0, 1, 63, 64, 65, 255, 256, 257, 300 and 4095, the two 255 caps, the neighbour
    cases; shared with the GPU tests"""
    rng = np.random.default_rng(7)
    rnd = lambda n: bytes(rng.integers(48, 123, n, dtype=np.uint8))
    head, tail = rnd(300), rnd(300)
    names = [rnd(n) for n in (0, 1, 63, 64, 65, 255, 256, 257, 300, 4095)]
    names += [head + b"first", head + b"second:longer"]             # 300 shared leading bytes
    names += [b"x1" + tail, b"another" + tail]                      # 300 shared trailing bytes
    names += [b"same", b"same", b"same"]                            # identical neighbours
    names += [b"prefix:of:the:next", b"prefix", b"prefix:grown"]    # a prefix of the previous one, and the reverse
    names += [b"aaaa", b"aa", b"aXa", b"aa"]                        # the two overlap cases
    names += [b"", b"", b"@at+plus", b"sp ace\ttab", b"hi\xff\x80\xfe"]
    return names


def _self_test():
    # the worked example of the format's description
    names = [b"r1/ab", b"r2/ab", b"r2/ab", b"r"]
    lens, pres, sufs, mids = columns(names)
    assert (lens, pres, sufs) == ([5, 5, 5, 1], [0, 1, 5, 1], [0, 3, 0, 0]) and b"".join(mids) == b"r1/ab2"
    m, body = section(names)
    assert m == dict(n_reads=4, name_bytes=16, mid_bytes=6, payload_bytes=24)
    assert body == struct.pack("<4H", 5, 5, 5, 1) + bytes([0, 1, 5, 1]) + bytes([0, 3, 0, 0]) + b"r1/ab2" + bytes(2)
    assert expand(m, body) == names
    # the two overlap cases
    assert columns([b"aaaa", b"aa"])[1:] == ([0, 2], [0, 0], [b"aaaa", b""])
    assert columns([b"aXa", b"aa"])[1:] == ([0, 1], [0, 1], [b"aXa", b""])
    # the chain restarts every 64 reads
    same = [b"same"] * 66
    assert columns(same)[1][63:66] == [4, 0, 4]
    assert name_of(b"@a b\tc\r") == b"a b\tc" and name_of(b"@a b\tc\r", "id") == b"a" and name_of(b"@ x", "id") == b""
    assert names_of(b"@a\nAC\n+\nII\n@b c\r\nAC\r\n+\r\nII") == [b"a", b"b c"]


_self_test()
