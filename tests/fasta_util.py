"""The FASTA reader's rule (include/sbgpu.h, sbgpu_fasta_*) restated in plain Python, line by line and from the rule's text alone,
and the generators of the files the tests read.  Nothing here calls the library."""
import numpy as np

EMPTY, RAGGED, DUPLICATE, NONAME = 1, 2, 4, 8
SPACE = b" \t\n\v\f\r"                       # C's isspace


class LeadingText(Exception):
    """A non-empty line in front of the first header; .offset is its first byte."""

    def __init__(self, offset):
        Exception.__init__(self, "text at %d" % offset)
        self.offset = offset


def lines_of(data):
    """-> [(start, end of the line's own bytes, terminator bytes)]"""
    out, pos, n = [], 0, len(data)
    while pos < n:
        nl = data.find(b"\n", pos)
        if nl < 0:
            out.append((pos, n, 0))
            break
        if nl > pos and data[nl - 1:nl] == b"\r":
            out.append((pos, nl - 1, 2))
        else:
            out.append((pos, nl, 1))
        pos = nl + 1
    return out


def restate(data):
    """-> dict(names, seqs, offset, line_bases, line_width, flags, lines) of a file's bytes; raises LeadingText."""
    data = bytes(data)
    contigs, lines = [], lines_of(data)
    for start, end, term in lines:
        if end > start and data[start:start + 1] == b">":
            name = data[start + 1:end]
            cut = [k for k in range(len(name)) if name[k:k + 1] in [SPACE[j:j + 1] for j in range(len(SPACE))]]
            contigs.append({"name": name[:cut[0]] if cut else name, "offset": end + term, "lines": []})
        elif not contigs:
            if end > start:
                raise LeadingText(start)
        else:
            contigs[-1]["lines"].append((data[start:end], term))
    out = {"names": [], "seqs": [], "offset": [], "line_bases": [], "line_width": [], "flags": [], "lines": len(lines)}
    seen = set()
    for c in contigs:
        seq = b"".join(text for text, _ in c["lines"])
        shape = [(len(text), term) for text, term in c["lines"]]
        lb, lw, flag = 0, 0, 0
        if not seq:
            flag |= EMPTY
        else:
            lb, lw = shape[0][0], shape[0][0] + shape[0][1]
            i = 0
            while i < len(shape) and shape[i] == shape[0]:
                i += 1
            if i < len(shape) and 1 <= shape[i][0] <= lb:
                i += 1
            while i < len(shape) and shape[i][0] == 0:
                i += 1
            if i < len(shape):
                flag |= RAGGED
        if not c["name"]:
            flag |= NONAME
        if c["name"].lower() in seen:      # (bytes.lower folds ASCII only)
            flag |= DUPLICATE
        seen.add(c["name"].lower())
        out["names"].append(c["name"]), out["seqs"].append(seq), out["offset"].append(c["offset"])
        out["line_bases"].append(lb), out["line_width"].append(lw), out["flags"].append(flag)
    return out


def fai_of(r):
    """The .fai text of a restatement without RAGGED or NONAME contigs."""
    return "".join("%s\t%d\t%d\t%d\t%d\n" % (n.decode("latin-1"), len(s), o, b, w)
                   for n, s, o, b, w, f in zip(r["names"], r["seqs"], r["offset"], r["line_bases"], r["line_width"], r["flags"]) if not f & EMPTY)


# ---- the CPU cases: name -> bytes.  Every name says what the file has.
def bases(n, seed=0):
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.choice(np.frombuffer(b"ACGTacgtN", np.uint8), size=n).tobytes()


def wrap(seq, width, term=b"\n", last=True):
    parts = [seq[i:i + width] for i in range(0, len(seq), width)]
    text = term.join(parts)
    return text + (term if last and parts else b"")


def cpu_cases():
    s = bases(400, 1)
    c = {}
    c["lf"] = b">chr1 first\n" + wrap(s[:150], 60) + b">chr2\n" + wrap(s[150:270], 60)
    c["crlf"] = b">chr1 first\r\n" + wrap(s[:150], 60, b"\r\n") + b">chr2\r\n" + wrap(s[150:270], 60, b"\r\n")
    c["no_final_newline"] = b">a\n" + wrap(s[:150], 60, last=False)
    c["no_final_newline_crlf"] = b">a\r\n" + wrap(s[:150], 60, b"\r\n", last=False)
    c["short_last_line"] = b">a\n" + wrap(s[:125], 60) + b">b\n" + wrap(s[:61], 60)
    c["blank_lines_behind"] = b">a\n" + wrap(s[:125], 60) + b"\n\r\n\n>b\n" + wrap(s[:120], 60) + b"\n\n"
    c["empty_header_header"] = b">a\n>b\n" + wrap(s[:70], 60)
    c["empty_at_end"] = b">a\n" + wrap(s[:70], 60) + b">b\n"
    c["empty_at_end_no_newline"] = b">a\n" + wrap(s[:70], 60) + b">b"
    c["empty_only_blank_lines"] = b">a\n\n\r\n>b\nAC\n"
    c["noname"] = b">\nACGT\n> described only\nACGT\n>x\nAC\n"
    c["duplicate"] = b">a\nAC\n>b\nGT\n>a\nTT\n"
    c["duplicate_by_case"] = b">Chr1\nAC\n>chr1 again\nGT\n>CHR1\nT\n"
    c["ragged_short_middle"] = b">a\n" + s[:60] + b"\n" + s[60:100] + b"\n" + s[100:160] + b"\n"
    c["ragged_long_last"] = b">a\n" + s[:60] + b"\n" + s[60:130] + b"\n"
    c["ragged_empty_first"] = b">a\n\n" + s[:60] + b"\n"
    c["ragged_empty_first_crlf"] = b">a\r\n\r\n" + s[:60] + b"\r\n"
    c["ragged_terminator_changes"] = b">a\n" + s[:60] + b"\n" + s[60:120] + b"\r\n" + s[120:180] + b"\n"
    c["ragged_terminator_changes_crlf"] = b">a\r\n" + s[:60] + b"\r\n" + s[60:120] + b"\n" + s[120:180] + b"\r\n"
    c["ragged_short_with_cr_keeps_width"] = b">a\n" + s[:60] + b"\n" + s[60:119] + b"\r\n" + s[119:179] + b"\n"
    c["ragged_empty_line_inside"] = b">a\n" + s[:60] + b"\n\n" + s[60:120] + b"\n"
    c["ragged_two_short_lines"] = b">a\n" + s[:60] + b"\n" + s[60:70] + b"\n" + s[70:75] + b"\n"
    c["last_full_line_other_terminator"] = b">a\n" + s[:60] + b"\n" + s[60:120] + b"\r\n\n"
    c["unwrapped"] = b">a\n" + s + b"\n>b\n" + s[:77]
    c["lone_cr_in_line"] = b">a\nAC\rGT\nACTGA\n>b\nAC\r\rGT\r\r\n"
    c["cr_last_byte"] = b">a\nACGT\r"
    c["nul_bytes"] = b">a\x00b c\nAC\x00T\nGG\n"
    c["name_ends"] = b">a\tb\nA\n>c\vd\nC\n>e\ff\nG\n>g\rh\nT\n>i j\nA\n"
    c["blank_lines_in_front"] = b"\n\r\n\n>a\nACGT\n"
    c["greater_inside_line"] = b">a\nAC>GT\n>b>c d\nA>\n"
    c["zero_bytes"] = b""
    c["only_empty_lines"] = b"\n\r\n\n\n"
    c["header_only"] = b">"
    c["many_small"] = many_contigs(200, seed=3)
    return c


def refused_cases():
    """name -> (bytes, the offset the refusal names)"""
    return {"text_first": (b"ACGT\n>a\nAC\n", 0), "text_behind_blank": (b"\n\r\nAC\n>a\nAC\n", 3), "no_header": (b"\nACGT", 1),
            "lone_cr_line": (b"\n\r\r\n>a\nA\n", 1), "cr_at_end": (b"\n\r", 1)}


def many_contigs(n, seed=0, lo=1, hi=100):
    """n contigs of lo .. hi bases, wrapped at random widths -- one in four at two widths, first the narrower: RAGGED where the
    second part has a full line -- so that a tile holds many headers."""
    rng = np.random.Generator(np.random.PCG64(seed))
    s = bases(hi, seed + 1)
    parts = []
    for k in range(n):
        ln, width = int(rng.integers(lo, hi + 1)), int(rng.integers(1, 80))
        half = ln // 2 if rng.integers(0, 4) == 0 else ln
        parts.append(b">c%d\n" % k + wrap(s[:half], width) + wrap(s[half:ln], width + 3))
    return b"".join(parts)


# ---- files at the device form's thresholds
def filler(n, width=60):
    """n >= 2 bytes of full sequence lines that end in '\\n' (the last line may be shorter)."""
    assert n >= 2
    q, r = divmod(n, width + 1)
    if r == 1:                   # a last line of 0 bases would be an empty line: the line in front gives one base up
        assert q >= 1
        return (b"A" * width + b"\n") * (q - 1) + b"A" * (width - 1) + b"\n" + b"C\n"
    return (b"A" * width + b"\n") * q + (b"G" * (r - 1) + b"\n" if r else b"")


def wrapped_file(n_bytes, width=60, name=b"s"):
    """exactly n_bytes bytes: one header, then lines of `width` bases; the last byte is whatever falls there"""
    head = b">" + name + b"\n"
    body = n_bytes - len(head)
    assert body >= 0
    line = b"ACGTTGCA" * (width // 8 + 1)
    text = (line[:width] + b"\n") * (body // (width + 1) + 1)
    return head + text[:body]


def header_at(pos, header_line, tail=b"ACGT\nAC\n"):
    """a contig `a` in front, then `header_line` (with its '\\n') beginning at byte `pos`"""
    return b">a\n" + filler(pos - 3) + header_line + tail


def crlf_split_at(pos):
    """a CRLF file whose '\\r' is byte pos - 1 and whose '\\n' is byte pos"""
    for k in range(1, 64):
        if (pos - 1 - 60 - (k + 3)) % 62 == 0:
            lines = (pos - 1 - 60 - (k + 3)) // 62 + 3
            return b">" + b"a" * k + b"\r\n" + (b"ACGTACGTAC" * 6 + b"\r\n") * lines
    raise AssertionError(pos)


def unwrapped(n_bases, final_newline):
    """a short contig, then one of n_bases bases on one line"""
    return b">u\nACGT\n>long one\n" + (b"ACGGT" * (n_bases // 5 + 1))[:n_bases] + (b"\n" if final_newline else b"")


def small_contigs(n):
    """n contigs of 4 bases"""
    return b"".join(b">%d\nACGT\n" % k for k in range(n))


def blocks_file(n_bytes, block_bases=100003, width=60):
    """at least n_bytes bytes of whole contigs of block_bases bases each"""
    block = wrap((b"ACGTTGCAAC" * (block_bases // 10 + 1))[:block_bases], width)
    n = n_bytes // (len(block) + 8) + 1
    return b"".join(b">b%05d\n" % k + block for k in range(n))
