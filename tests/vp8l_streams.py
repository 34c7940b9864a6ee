"""Directed VP8L streams: the pin of the RFC 9649 stream decoder (host/vp8_alpha.c: code_build, code_read,
code_parse, image_decode, lossless_entropy) and of everything it feeds (vp8g_make_lossless_desc and the
lossless kernel, the ALPH path, the batch pipeline).

Every other lossless stream of the suite was written by libwebp 1.2.2's encoder, which never sends a prefix code
longer than the table's 8 bits on a small picture, a code of one leaf in its normal form, code 16 as the first
code-length symbol, an explicit max_symbol in most of its field widths, most of the 120 plane codes at a narrow
width, an unused prefix-code group, predictor modes 0 / 13 / 14 / 15, or block bits other than 2, 3 and 6.  Here
a test-only writer spells a stream out bit by bit from a case that says what is written: prefix codes as explicit
length arrays (canonical code assignment as in the RFC) in the simple or the normal form -- with a chosen count of
code-length-code lengths, chosen use of 16 / 17 / 18 and an optional max_symbol of a chosen field width --, the
image as a list of tokens

    ("lit", argb)   ("idx", cache index)   ("copy", length, distance code: a plane code 1..120, or 120 + distance)

with the group of every token taken from an optional entropy image, the transforms with their data written as
sub-images the same way, and a container around it (bare payload, RIFF/WEBP/VP8L, VP8X + VP8L, or a headerless
stream behind an ALPH header byte).  Where a case leaves a code open, the writer fills in the flat code over the
symbols the tokens use (one symbol: the simple form; two below 256: the simple form; else lengths k - 1 and k) --
a fixed rule, not a search.

The expected picture is not read back from the bits: build() expands the token list (the colour cache, the
distance map derived from its ordering rule, overlapping copies) and applies the transforms' meaning in plain
Python integers / numpy.  tests/golden/vp8l_kat.json (make_vp8l_kat.py) holds libwebp's verdict and RGBA hash for
every stream as the second witness.

CASES is the one table: name -> a function returning the case dict
  w, h        picture size
  image       dict(tokens, cache_bits, codes, meta, ...) of the spatially coded image (at the packed width)
  transforms  list of dicts in stream order: type P / CC / SG / CI, bits, data (uint32 [bh, bw]) or table
  container   "riff" (default) / "vp8x" / "alph"; alph: filter
  refuse      True: the stream is meant to be refused (the nearest refused neighbour of an accepted case)
  cut         bytes taken off the end
build(name) -> Built(name, data, payload, argb, alpha, census, features, ...); everything is seeded and cached.
"""
import collections
import functools
import hashlib
import pathlib
import struct
import zlib

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden"

P, CC, SG, CI = 0, 1, 2, 3
TYPE_NAMES = ("predictor", "cross_color", "subtract_green", "color_index")
ALPHABETS = (256 + 24, 256, 256, 256, 40)
CL_ORDER = (17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)
CENSUS = ("lossless", "predictor", "cross_color", "subtract_green", "color_index", "pack_bits_1", "pack_bits_2", "pack_bits_4",
          "pack_bits_8", "multi_group", "backrefs", "short_dist", "cache_hits", "simple_codes", "normal_codes", "repeat_16",
          "repeat_17", "repeat_18")  # (the fields of Vp8fAlphaStats a lossless stream moves; "literals" is the writer's own)
ALPH_BASE = "ll_levels2_f3"  # the 67 x 45 lossy fixture of tests/golden/alpha/ whose VP8 chunk carries the ALPH cases
ALPH_W, ALPH_H = 67, 45


# ---- bits -------------------------------------------------------------------------------------------------

class Bits:
    """LSB-first bit writer (RFC 9649 3.1: ReadBits takes the least significant bit of a byte first)."""

    def __init__(self):
        self.out, self.acc, self.fill, self.nbits = bytearray(), 0, 0, 0

    def put(self, value: int, n: int):
        assert n >= 0 and 0 <= value < (1 << n) or (n == 0 and value == 0), (value, n)
        self.acc |= value << self.fill
        self.fill += n
        self.nbits += n
        while self.fill >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.fill -= 8

    def bytes(self) -> bytes:
        return bytes(self.out) + (bytes([self.acc]) if self.fill else b"")


# ---- prefix codes ---------------------------------------------------------------------------------------------

def simple(*syms, first8=None):
    """The simple form: one or two symbols; first8: the first symbol's field is 8 bits wide (default: only if it
    has to be)."""
    assert 1 <= len(syms) <= 2
    return {"kind": "simple", "syms": tuple(syms), "first8": first8}


def normal(lengths=None, *, ops=None, ncl=None, cl=None, max_symbol=None):
    """The normal form.  lengths: {symbol: length}, written with zero runs of 3 or more as 17 / 18 and everything
    else literally; or ops: the code-length symbols themselves, ("lit", v) / (16, run) / (17, run) / (18, run).
    ncl: how many code-length-code lengths are sent (default: as few as the format allows); cl: {code-length
    symbol: length} of the code-length code (default: flat over the symbols in use); max_symbol: (value, k) =
    the count of code-length symbols to read, in a field of 2 + 2 k bits."""
    assert (lengths is None) != (ops is None)
    return {"kind": "normal", "lengths": lengths, "ops": ops, "ncl": ncl, "cl": cl, "max_symbol": max_symbol}


def flat(symbols):
    """{symbol: length} of the complete code over `symbols` whose lengths differ by one at most; the first ones in
    value order are the shorter."""
    s = sorted(set(symbols))
    if len(s) == 1:
        return {s[0]: 1}
    k = (len(s) - 1).bit_length()
    short = (1 << k) - len(s)
    return {v: k - 1 if i < short else k for i, v in enumerate(s)}


def canonical(lengths: dict) -> dict:
    """{symbol: (code, length)}: codes in increasing order by (length, symbol), a length's first code the last one
    of the length before plus one, shifted (RFC 9649 3.7.2.1.1 by way of RFC 1951 3.2.2)."""
    out, code = {}, 0
    for l in range(1, 16):
        for s in sorted(v for v, n in lengths.items() if n == l):
            out[s] = (code & ((1 << l) - 1), l)
            code += 1
        code <<= 1
    return out


def ops_of(lengths: dict, alphabet: int):
    ops, s = [], 0
    while s < alphabet:
        if lengths.get(s, 0):
            ops.append(("lit", lengths[s]))
            s += 1
            continue
        run = 0
        while s + run < alphabet and not lengths.get(s + run, 0):
            run += 1
        s += run
        while run >= 3:
            n = min(run, 138)
            ops.append((18, n) if n >= 11 else (17, n))
            run -= n
        ops += [("lit", 0)] * run
    return ops


def lengths_of(ops, alphabet: int):
    """What the code-length symbols mean: 16 repeats the last non-zero length (8 before there is one) 3..6 times,
    17 and 18 write 3..10 and 11..138 zeros.  None if they run past the alphabet."""
    out, prev = [], 8
    for op, n in ops:
        if op == "lit":
            out.append(n)
            prev = n or prev
        else:
            out += [prev if op == 16 else 0] * n
        if len(out) > alphabet:
            return None
    return {s: l for s, l in enumerate(out) if l}


def kraft(lengths: dict):
    return sum(1 << (15 - l) for l in lengths.values()) - (1 << 15)  # 0: complete, < 0: incomplete, > 0: over-subscribed


class Writer:
    def __init__(self):
        self.b = Bits()
        self.census = collections.Counter()
        self.features = set()
        self.valid = True  # (cleared when the writer itself sees that the stream cannot decode)

    def symbol(self, table: dict, sym: int):
        """One symbol of the code `table` ({symbol: (code, length)}); a code of one leaf costs no bits.  The code's
        most significant bit goes first."""
        if len(table) == 1:
            assert sym in table
            return
        code, l = table[sym]
        for i in range(l - 1, -1, -1):
            self.b.put((code >> i) & 1, 1)
        if l > 8:
            self.features.add(("code_longer_than_8", l))

    def code(self, spec: dict, alphabet: int, where: str) -> dict:
        """Write one prefix code; returns its {symbol: (code, length)}."""
        b, f = self.b, self.features
        if spec["kind"] == "simple":
            syms = spec["syms"]
            first8 = spec["first8"] if spec["first8"] is not None else syms[0] > 1
            b.put(1, 1)
            b.put(len(syms) - 1, 1)
            b.put(int(first8), 1)
            b.put(syms[0], 8 if first8 else 1)
            if len(syms) == 2:
                b.put(syms[1], 8)
                f.add("simple_two_8bit_first" if first8 else "simple_two_1bit_first")
                if syms[0] == syms[1]:
                    f.add("simple_same_symbol")
            else:
                f.add("simple_one_8bit" if first8 else "simple_one_1bit")
            self.census["simple_codes"] += 1
            if max(syms) >= alphabet:
                self.valid = False
            elif max(syms) == min(alphabet, 256) - 1:
                f.add(("simple_top_symbol", where))
            return canonical({s: 1 for s in syms})
        ops = spec["ops"] if spec["ops"] is not None else ops_of(spec["lengths"], alphabet)
        used = sorted({n if op == "lit" else op for op, n in ops})
        cl = spec["cl"] if spec["cl"] is not None else flat(used)
        ncl = spec["ncl"] or max(4, 1 + max(CL_ORDER.index(s) for s in cl))
        assert all(CL_ORDER.index(s) < ncl for s in cl) and 4 <= ncl <= 19
        b.put(0, 1)
        b.put(ncl - 4, 4)
        for s in CL_ORDER[:ncl]:
            b.put(cl.get(s, 0), 3)
        f.add(("code_length_lengths", ncl))
        cl_ok = len(cl) == 1 or kraft(cl) == 0
        if len(cl) == 1 and cl_ok:
            f.add(("code_length_code_one_leaf", next(iter(cl))))
        ctab = canonical(cl)
        total = sum(1 if op == "lit" else n for op, n in ops)
        if spec["max_symbol"]:
            value, k = spec["max_symbol"]
            b.put(1, 1)
            b.put(k, 3)
            b.put(value - 2, 2 + 2 * k)
            f.add(("max_symbol_width", k))
            if value == 2:
                f.add("max_symbol_2")
            if value == alphabet:
                f.add("max_symbol_alphabet")
            if value > alphabet:
                self.valid = False
            elif total < alphabet:
                f.add("max_symbol_runs_out")
            assert value == len(ops) or value > alphabet
        else:
            b.put(0, 1)
        s = 0
        for i, (op, n) in enumerate(ops):
            sym = n if op == "lit" else op
            if sym in ctab:
                self.symbol(ctab, sym)
            if op == "lit":
                s += 1
                continue
            lo, width = {16: (3, 2), 17: (3, 3), 18: (11, 7)}[op]
            b.put(n - lo, width)
            self.census[f"repeat_{op}"] += 1
            f.add((f"repeat_{op}", n))
            if op == 16 and i == 0:
                f.add("repeat_16_first")
            if op == 16 and i >= 2 and ops[i - 1] in (("lit", 0), (17, ops[i - 1][1]), (18, ops[i - 1][1])):
                first = next((m for o, m in ops[:i] if o == "lit" and m), None)
                if first not in (None, 8):
                    f.add("repeat_16_after_zeros")
            s += n
            if s == alphabet and i == len(ops) - 1:
                f.add("run_ends_at_alphabet_end")
        self.census["normal_codes"] += 1
        lengths = lengths_of(ops, alphabet)
        if lengths is None or not cl_ok or not lengths or (len(lengths) > 1 and kraft(lengths) != 0):
            self.valid = False
            return canonical(lengths or {0: 1})
        if len(lengths) == 1:
            f.add(("normal_one_symbol", next(iter(lengths.values()))))
        if {8, 9} <= set(lengths.values()):
            f.add("lengths_8_and_9")
        return canonical(lengths)


# ---- images ---------------------------------------------------------------------------------------------------

def dist_map():
    """The 120 (xi, yi) of the short-distance codes (RFC 9649 5.2.2): the neighbourhood yi = 0, xi = 1..8 and
    yi = 1..7, xi = -7..8, in order of Euclidean distance; ties by |xi|, then the positive xi first."""
    cells = [(x, 0) for x in range(1, 9)] + [(x, y) for y in range(1, 8) for x in range(-7, 9)]
    return sorted(cells, key=lambda c: (c[0] * c[0] + c[1] * c[1], abs(c[0]), c[0] < 0))


DIST_MAP = dist_map()
assert len(DIST_MAP) == 120 and DIST_MAP[:4] == [(0, 1), (1, 0), (1, 1), (-1, 1)] and DIST_MAP[-1] == (8, 7)


def prefix_symbol(v: int):
    """(symbol, extra bit count, extra bits) of the length or distance code v >= 1 (RFC 9649 5.2.2)."""
    if v <= 4:
        return v - 1, 0, 0
    d = v - 1
    hb = d.bit_length() - 1
    return 2 * hb + ((d >> (hb - 1)) & 1), hb - 1, d & ((1 << (hb - 1)) - 1)


def cache_slot(p: int, bits: int) -> int:
    return ((0x1E35A7BD * p) & 0xFFFFFFFF) >> (32 - bits)


def lits(pixels):
    return [("lit", int(p)) for p in np.asarray(pixels, dtype=np.uint32).reshape(-1)]


def image(tokens, cache_bits=0, codes=None, meta=None, ngroups=None, meta_codes=None, cache_raw=None):
    """meta: (tile bits, [[group index]] of the entropy image); codes: per group five specs (None: the flat code
    over what the tokens use); ngroups: groups in the stream (default: the highest index used + 1); cache_raw:
    (flag, bits) written as they stand."""
    return {"tokens": tokens, "cache_bits": cache_bits, "codes": codes or {}, "meta": meta, "ngroups": ngroups,
            "meta_codes": meta_codes, "cache_raw": cache_raw}


def auto_code(used):
    u = sorted(used)
    if not u:
        return simple(0)
    if len(u) == 1:
        return simple(u[0]) if u[0] < 256 else normal({u[0]: 1})
    if len(u) == 2 and u[1] < 256:
        return simple(u[0], u[1])
    return normal(flat(u))


def write_image(wr: Writer, img: dict, w: int, h: int, level0: bool, where: str):
    """Write one entropy-coded image; returns its pixels (list of w * h ints), or None if the tokens themselves
    are invalid."""
    b, f = wr.b, wr.features
    cache_bits = img["cache_bits"]
    if img["cache_raw"]:
        b.put(img["cache_raw"][0], 1)
        b.put(img["cache_raw"][1], 4)
        wr.valid = False
    elif cache_bits:
        b.put(1, 1)
        b.put(cache_bits, 4)
        if level0:
            f.add(("cache_bits", cache_bits))
    else:
        b.put(0, 1)
    meta, mbits, gmap = img["meta"], 0, None
    if level0:
        if meta:
            mbits, gmap = meta
            mw, mh = (w + (1 << mbits) - 1) >> mbits, (h + (1 << mbits) - 1) >> mbits
            assert len(gmap) == mh and all(len(r) == mw for r in gmap)
            b.put(1, 1)
            b.put(mbits - 2, 3)
            junk = np.random.default_rng(mw * 31 + mh) if not img["meta_codes"] else None  # (blue and alpha are not read)
            px = [(g >> 8) << 16 | (g & 255) << 8 | (int(junk.integers(0, 4)) | int(junk.integers(0, 4)) << 24 if junk else 0)
                  for r in gmap for g in r]
            sub = image(lits(px), codes={0: img["meta_codes"]} if img["meta_codes"] else None)
            write_image(wr, sub, mw, mh, False, "meta")
            f.add(("meta_bits", mbits))
            if w % (1 << mbits):
                f.add("meta_width_not_multiple_of_tile")
            if max(g for r in gmap for g in r) > 255:
                f.add("group_above_255")
        else:
            b.put(0, 1)
    used_groups = sorted({g for r in gmap for g in r}) if gmap else [0]
    ngroups = img["ngroups"] or used_groups[-1] + 1
    if ngroups > 1:
        wr.census["multi_group"] += 1
    if len(used_groups) < ngroups:
        f.add(("unused_groups", ngroups - len(used_groups)))
    # pass 1: the group and the symbols of every token, and the pixels they mean
    n = w * h
    pix, cache = [], [0] * (1 << cache_bits) if cache_bits else None
    written, by_copy = set(), set()  # slots written at all / whose present colour only a copy put there
    usage = collections.defaultdict(lambda: [set() for _ in range(5)])
    plan, ok = [], True
    last_group = None
    for tok in img["tokens"]:
        pos = len(pix)
        if pos >= n:
            ok = False
            break
        x, y = pos % w, pos // w
        g = gmap[y >> mbits][x >> mbits] if gmap else 0
        if last_group is not None and g != last_group and x != 0:
            f.add("group_changes_mid_row")
        last_group = g
        u = usage[g]
        if tok[0] == "lit":
            p = tok[1]
            for k, s in enumerate(((p >> 8) & 255, (p >> 16) & 255, p & 255, p >> 24)):
                u[k].add(s)
            plan.append((g, "lit", p))
            pix.append(p)
            if cache is not None:
                slot = cache_slot(p, cache_bits)
                if slot in written and cache[slot] != p:
                    f.add(("cache_collision", cache_bits))
                cache[slot] = p
                written.add(slot)
                by_copy.discard(slot)
            wr.census["literals"] += 1
        elif tok[0] == "idx":
            i = tok[1]
            u[0].add(256 + 24 + i)
            plan.append((g, "idx", i))
            if cache is None or i >= len(cache):
                ok = False
                break
            v = cache[i]
            pix.append(v)
            wr.census["cache_hits"] += 1
            if i not in written:
                f.add("cache_slot_never_written")
            if i in by_copy:
                f.add("cache_hit_entered_by_copy")
            cache[cache_slot(v, cache_bits)] = v  # (every pixel enters the cache: 0 from an empty slot goes to slot 0)
            written.add(cache_slot(v, cache_bits))
            if i == len(cache) - 1:
                f.add(("cache_last_index", cache_bits))
        else:
            _, length, dcode = tok
            ls, lx, lv = prefix_symbol(length)
            ds, dx, dv = prefix_symbol(dcode)
            u[0].add(256 + ls)
            u[4].add(ds)
            plan.append((g, "copy", (ls, lx, lv, ds, dx, dv)))
            if dcode > 120:
                dist = dcode - 120
            else:
                xi, yi = DIST_MAP[dcode - 1]
                dist = xi + yi * w
                wr.census["short_dist"] += 1
                f.add(("plane_code", w, dcode))
                if dist < 1:
                    f.add(("plane_code_clamped", "zero" if dist == 0 else "negative"))
                    dist = 1
            wr.census["backrefs"] += 1
            if ds >= 40 or dist > pos or length > n - pos:
                ok = False
                break
            if dist < length:
                f.add("copy_overlaps")
            if x + length > w:
                f.add("copy_crosses_row_end")
            if x + length > 2 * w:
                f.add("copy_crosses_several_row_ends")
            if pos + length == n:
                f.add("copy_ends_on_last_pixel")
            if ls == 23:
                f.add("longest_length_symbol")
            f.add(("distance_symbol", ds))
            if gmap:
                e = pos + length - 1
                if gmap[(e // w) >> mbits][(e % w) >> mbits] != g or any(
                        gmap[(q // w) >> mbits][(q % w) >> mbits] != g for q in range(pos, pos + length)):
                    f.add("copy_crosses_tile")
            for _ in range(length):
                p = pix[len(pix) - dist]
                pix.append(p)
                if cache is not None:
                    slot = cache_slot(p, cache_bits)
                    if cache[slot] != p:  # (this copy, and nothing else, puts p there)
                        by_copy.add(slot)
                    cache[slot] = p
                    written.add(slot)
    if len(pix) != n:
        ok = False
    # the codes: the case's own, else the flat code over what the group's tokens use
    tables = {}
    for g in range(ngroups):
        given = img["codes"].get(g) or [None] * 5
        tabs = []
        for k in range(5):
            spec = given[k] or auto_code(usage[g][k] if g in usage else ())
            before = wr.valid
            tabs.append(wr.code(spec, ALPHABETS[k] + ((1 << cache_bits) if k == 0 and cache_bits else 0), f"{where}:{'grbad'[k]}"))
            if g not in usage and before and not wr.valid:  # (no token reads it: whether that refuses the stream is the decoder's call)
                wr.valid = True
                f.add("invalid_code_in_unused_group")
        tables[g] = tabs
    bits0 = b.nbits
    for g, kind, v in plan:
        t = tables[g]
        if kind == "lit":
            for k, s in enumerate(((v >> 8) & 255, (v >> 16) & 255, v & 255, v >> 24)):
                if s not in t[k]:
                    wr.valid = False  # (an invalid code of the case's own: nothing after it is read)
                    return None
                wr.symbol(t[k], s)
        elif kind == "idx":
            wr.symbol(t[0], 256 + 24 + v)
        else:
            ls, lx, lv, ds, dx, dv = v
            wr.symbol(t[0], 256 + ls)
            b.put(lv, lx)
            if ds in t[4]:
                wr.symbol(t[4], ds)
            b.put(dv, dx)
    if b.nbits == bits0 and level0:
        f.add("pixel_data_of_zero_bits")
    if not ok:
        wr.valid = False
        return None
    return pix


# ---- the transforms' meaning ---------------------------------------------------------------------------------

def _ch(p):
    return [(p >> s) & 255 for s in (0, 8, 16, 24)]


def _px(c):
    return sum((int(v) & 255) << s for v, s in zip(c, (0, 8, 16, 24)))


def _avg(a, b):
    return _px([(x + y) >> 1 for x, y in zip(_ch(a), _ch(b))])


def _clip(v):
    return 0 if v < 0 else 255 if v > 255 else v


def _predict(mode, L, T, TL, TR):
    """RFC 9649 4.1: the fourteen predictors; the modes the RFC leaves undefined (14, 15) are opaque black, which is
    how libwebp reads them."""
    if mode == 1:
        return L
    if mode == 2:
        return T
    if mode == 3:
        return TR
    if mode == 4:
        return TL
    if mode == 5:
        return _avg(_avg(L, TR), T)
    if mode == 6:
        return _avg(L, TL)
    if mode == 7:
        return _avg(L, T)
    if mode == 8:
        return _avg(TL, T)
    if mode == 9:
        return _avg(T, TR)
    if mode == 10:
        return _avg(_avg(L, TL), _avg(T, TR))
    if mode == 11:  # Select: the Manhattan distances of L + T - TL to L and to T
        pl = sum(abs(t - tl) for t, tl in zip(_ch(T), _ch(TL)))
        pt = sum(abs(l - tl) for l, tl in zip(_ch(L), _ch(TL)))
        return L if pl < pt else T
    if mode == 12:
        return _px([_clip(l + t - tl) for l, t, tl in zip(_ch(L), _ch(T), _ch(TL))])
    if mode == 13:
        a = _avg(L, T)
        return _px([_clip(x + int((x - tl) / 2)) for x, tl in zip(_ch(a), _ch(TL))])  # (division towards zero)
    return 0xFF000000


def _add(a, b):
    return _px([x + y for x, y in zip(_ch(a), _ch(b))])


def inv_predictor(pix, w, h, bits, modes):
    out = list(pix)
    for y in range(h):
        for x in range(w):
            i = y * w + x
            if y == 0:
                pred = 0xFF000000 if x == 0 else out[i - 1]
            elif x == 0:
                pred = out[i - w]
            else:  # (the rightmost pixel's TR is the leftmost pixel of the row being decoded: memory order)
                pred = _predict((int(modes[y >> bits][x >> bits]) >> 8) & 15, out[i - 1], out[i - w], out[i - w - 1], out[i - w + 1])
            out[i] = _add(out[i], pred)
    return out


def _s8(v):
    return v - 256 if v > 127 else v


def inv_cross_color(pix, w, h, bits, data):
    out = []
    for y in range(h):
        for x in range(w):
            e = int(data[y >> bits][x >> bits])
            g2r, g2b, r2b = _s8(e & 255), _s8((e >> 8) & 255), _s8((e >> 16) & 255)
            b, g, r, a = _ch(pix[y * w + x])
            r = (r + ((g2r * _s8(g)) >> 5)) & 255
            b = (b + ((g2b * _s8(g)) >> 5)) & 255
            b = (b + ((r2b * _s8(r)) >> 5)) & 255
            out.append(_px([b, g, r, a]))
    return out


def inv_subtract_green(pix):
    return [_px([b + g, g, r + g, a]) for b, g, r, a in map(_ch, pix)]


def inv_color_index(pix, w, h, pack, table):
    pw, bpp = (w + (1 << pack) - 1) >> pack, 8 >> pack
    out = []
    for y in range(h):
        for x in range(w):
            i = (((pix[y * pw + (x >> pack)] >> 8) & 255) >> ((x & ((1 << pack) - 1)) * bpp)) & ((1 << bpp) - 1)
            out.append(table[i] if i < len(table) else 0)
    return out


def pack_bits(ncolors: int) -> int:
    return 0 if ncolors > 16 else 1 if ncolors > 4 else 2 if ncolors > 2 else 3


def unfilter(res, w, h, flt):
    """RFC 9649 2.7.1.2: the alpha plane from its residual under filter 0..3."""
    out = [0] * (w * h)
    for y in range(h):
        for x in range(w):
            i = y * w + x
            if flt == 0 or i == 0:
                pred = 0
            elif y == 0:
                pred = out[i - 1]
            elif x == 0:
                pred = out[i - w]
            elif flt == 1:
                pred = out[i - 1]
            elif flt == 2:
                pred = out[i - w]
            else:
                pred = _clip(out[i - 1] + out[i - w] - out[i - w - 1])
            out[i] = (pred + res[i]) & 255
    return out


# ---- containers -------------------------------------------------------------------------------------------------

def chunk(tag: bytes, payload: bytes) -> bytes:
    return tag + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b"")


def riff(body: bytes) -> bytes:
    return b"RIFF" + struct.pack("<I", len(body) + 4) + b"WEBP" + body


def vp8x(flags: int, w: int, h: int) -> bytes:
    return chunk(b"VP8X", bytes([flags, 0, 0, 0]) + struct.pack("<I", w - 1)[:3] + struct.pack("<I", h - 1)[:3])


F_ALPHA = 0x10


def alph_base_vp8() -> bytes:
    """The VP8 chunk (header and padding included) of the lossy fixture the ALPH cases ride on."""
    data = (GOLDEN / "alpha" / f"{ALPH_BASE}.webp").read_bytes()
    pos = 12
    while pos + 8 <= len(data):
        n = struct.unpack("<I", data[pos + 4:pos + 8])[0]
        if data[pos:pos + 4] == b"VP8 ":
            return data[pos:pos + 8 + n + (n & 1)]
        pos += 8 + n + (n & 1)
    raise ValueError("no VP8 chunk")


# ---- build ----------------------------------------------------------------------------------------------------

Built = collections.namedtuple("Built", "name data payload width height argb alpha census features transforms refuse valid container")


@functools.lru_cache(maxsize=None)
def build(name: str) -> Built:
    case = CASES[name]()
    w, h = case["w"], case["h"]
    container = case.get("container", "riff")
    wr = Writer()
    b, f = wr.b, wr.features
    xs, trs, seen = w, [], set()
    for t in case.get("transforms", ()):
        b.put(1, 1)
        b.put(t["type"], 2)
        if t["type"] in seen:
            wr.valid = False
        seen.add(t["type"])
        rec = {"type": t["type"], "bits": t.get("bits", 0), "xsize": xs, "ncolors": 0}
        if t["type"] in (P, CC):
            bits = t["bits"]
            b.put(bits - 2, 3)
            data = np.asarray(t["data"], dtype=np.uint32)
            bw, bh = (xs + (1 << bits) - 1) >> bits, (h + (1 << bits) - 1) >> bits
            assert data.shape == (bh, bw), (name, data.shape, (bh, bw))
            write_image(wr, image(lits(data)), bw, bh, False, "sub")
            rec["data"] = data
            wr.census[TYPE_NAMES[t["type"]]] += 1
            f.add(("predictor_bits" if t["type"] == P else "cross_color_bits", bits))
            if t["type"] == P:
                f.update(("predictor_mode", int(m)) for m in np.unique((data >> 8) & 15))
                if (data & 0xFFFF00FF).any():
                    f.add("mode_image_junk")
            if (w, h) == (1, 1):
                f.add(("transform_on_1x1", t["type"]))
        elif t["type"] == CI:
            table = [int(c) for c in t["table"]]
            nc = len(table)
            b.put(nc - 1, 8)
            deltas = [table[0]] + [_px([x - y for x, y in zip(_ch(table[i]), _ch(table[i - 1]))]) for i in range(1, nc)]
            if any(x < y for i in range(1, nc) for x, y in zip(_ch(table[i]), _ch(table[i - 1]))):
                f.add("table_deltas_wrap")
            write_image(wr, image(lits(deltas)), nc, 1, False, "table")
            rec["bits"], rec["ncolors"], rec["table"] = pack_bits(nc), nc, table
            f.add(("color_index_colors", nc))
            f.add(("color_index_width", xs))
            xs = (xs + (1 << rec["bits"]) - 1) >> rec["bits"]
            wr.census["color_index"] += 1
            wr.census[f"pack_bits_{8 >> rec['bits']}"] += 1
        else:
            wr.census["subtract_green"] += 1
        trs.append(rec)
    b.put(0, 1)
    f.add(("order", tuple(t["type"] for t in trs)))
    pix = write_image(wr, case["image"], xs, h, True, "main")
    if case.get("exact_end"):
        assert b.nbits % 8 == 0, (name, b.nbits)
        f.add("stream_ends_on_the_group_bound")
    wr.census["lossless"] += 1
    stream = b.bytes()
    if case.get("cut"):
        stream = stream[:len(stream) - case["cut"]]
        wr.valid = False
    argb = alpha = None
    if wr.valid and pix is not None:
        width = xs
        for t in reversed(trs):
            if t["type"] == P:
                pix = inv_predictor(pix, t["xsize"], h, t["bits"], t["data"])
            elif t["type"] == CC:
                pix = inv_cross_color(pix, t["xsize"], h, t["bits"], t["data"])
            elif t["type"] == SG:
                pix = inv_subtract_green(pix)
            else:
                if any(i >= t["ncolors"] for i in _indices(pix, t["xsize"], h, t["bits"])):
                    f.add("index_beyond_table")
                pix = inv_color_index(pix, t["xsize"], h, t["bits"], t["table"])
                width = t["xsize"]
        assert width == w
        argb = np.array(pix, dtype=np.uint32).reshape(h, w)
    census = {k: int(wr.census[k]) for k in CENSUS + ("literals",)}
    if container == "alph":
        flt = case["filter"]
        payload = bytes([flt << 2 | 1]) + stream
        data = riff(vp8x(F_ALPHA, w, h) + chunk(b"ALPH", payload) + alph_base_vp8())
        if argb is not None:
            alpha = np.array(unfilter([(p >> 8) & 255 for p in pix], w, h, flt), dtype=np.uint8).reshape(h, w)
            if (argb & 0xFFFF00FF).any():
                f.add("alph_junk_in_other_channels")
            f.add(("alph_filter", flt))
            f.update(("alph_transform", t["type"]) for t in trs)
    else:
        hint = int(argb is not None and bool(((argb >> 24) != 255).any()))
        payload = b"\x2f" + struct.pack("<I", (w - 1) | (h - 1) << 14 | hint << 28) + stream
        if container == "vp8x":
            data = riff(vp8x(F_ALPHA if hint else 0, w, h) + chunk(b"VP8L", payload))
        else:
            data = riff(chunk(b"VP8L", payload))
    f.add(("container", container))
    f.update(case.get("tags", ()))
    if case.get("refuse") is None and not wr.valid:
        raise AssertionError(f"{name}: the writer finds its own stream invalid")
    return Built(name, data, payload, w, h, argb, alpha, census, frozenset(f), trs, case.get("refuse"), wr.valid, container)


def _indices(pix, w, h, pack):
    pw, bpp = (w + (1 << pack) - 1) >> pack, 8 >> pack
    for y in range(h):
        for x in range(w):
            yield (((pix[y * pw + (x >> pack)] >> 8) & 255) >> ((x & ((1 << pack) - 1)) * bpp)) & ((1 << bpp) - 1)


def rgba(argb) -> bytes:
    a = np.asarray(argb, dtype=np.uint32)
    return np.stack([(a >> 16) & 255, (a >> 8) & 255, a & 255, a >> 24], axis=-1).astype(np.uint8).tobytes()


def sha(b: bytes) -> str:
    return hashlib.sha256(b).hexdigest()


# ---- the cases ------------------------------------------------------------------------------------------------

CASES = {}


def case(fn):
    CASES[fn.__name__] = fn
    return fn


def rng_of(name: str):
    return np.random.default_rng(zlib.crc32(name.encode()))


def pixels(name, n, levels=(4, 3, 3, 2)):
    """n seeded pixels with a few values per channel (green, red, blue, alpha), so that the flat codes stay short."""
    r = rng_of(name)
    vals = [r.choice(256, size=k, replace=False) for k in levels]
    g, rd, bl, a = (v[r.integers(0, len(v), n)].astype(np.uint32) for v in vals)
    return [int(p) for p in (a << 24 | rd << 16 | g << 8 | bl)]


W0, H0 = 8, 4  # the picture of the prefix-code cases


def with_code(name, k, spec, need=None, **kw):
    """The 8 x 4 picture whose channel k (0 green, 1 red, 2 blue, 3 alpha, 4 distance) is written under `spec`;
    need: the values that channel takes."""
    px = pixels(name, W0 * H0)
    if need is not None and k < 4:
        sh = (8, 16, 0, 24)[k]
        r = rng_of(name + "/need")
        px = [(p & ~(255 << sh)) | int(need[r.integers(0, len(need))]) << sh for p in px]
        for i, v in enumerate(need):  # (every value at least once)
            px[i] = (px[i] & ~(255 << sh)) | int(v) << sh
    codes = [None] * 5
    codes[k] = spec
    return dict(w=W0, h=H0, image=image(lits(px), codes={0: codes}), **kw)


# -- prefix codes: simple codes that cost no bits

@case
def zero_bits_1x1():
    return dict(w=1, h=1, image=image([("lit", 0x80C04020)]))


@case
def zero_bits_3x2():
    return dict(w=3, h=2, image=image([("lit", 0xFF010001)] * 6))


def _two_groups():
    # 5 x 1 under 4-pixel tiles: two groups of five 4-bit simple codes each, no pixel bits; the entropy image's own
    # codes take the 8-bit symbol field so that the stream ends on a byte: exactly ngroups * 20 bits are left
    m8 = [simple(0, 1, first8=True)] + [simple(v, first8=True) for v in (0, 0, 0, 0)]
    return image([("lit", 0x01000100)] * 4 + [("lit", 0x00010001)], meta=(2, [[0, 1]]), meta_codes=m8)


@case
def zero_bits_two_groups_on_the_bound():
    im = _two_groups()
    return dict(w=5, h=1, image=im, exact_end=True)


@case
def zero_bits_two_groups_one_short():
    return dict(w=5, h=1, image=_two_groups(), cut=1, refuse=True)


# -- other simple forms

@case
def simple_two_8bit_first():
    return with_code("simple_two_8bit_first", 1, simple(200, 37), need=[200, 37])


@case
def simple_same_symbol():
    c = with_code("simple_same_symbol", 2, simple(5, 5), need=[5])
    c["image"]["codes"][0][3] = simple(1, 1)
    c["image"]["tokens"] = [("lit", (p & 0x00FFFFFF) | 0x01000000) for _, p in c["image"]["tokens"]]
    return c


@case
def simple_top_symbols():
    px = [(p & 0xFF00FF00) | 0xFF | (255 << 16 if i & 1 else 254 << 16) for i, p in enumerate(pixels("simple_top_symbols", W0 * H0))]
    px = [(p & 0x00FF00FF) | 0xFF000000 | 0xFF00 for p in px]
    codes = [simple(255), simple(254, 255), simple(255), simple(255), simple(38, 39)]
    return dict(w=W0, h=H0, image=image(lits(px), codes={0: codes}))


@case
def simple_distance_40():
    return with_code("simple_distance_40", 4, simple(40), refuse=True)


# -- normal codes

def _one_symbol(name, length):
    c = with_code(name, 1, normal({77: length}), need=[77])
    c["image"]["codes"][0][0] = normal({130: length})
    c["image"]["tokens"] = [("lit", (p & 0xFFFF00FF) | 130 << 8) for _, p in c["image"]["tokens"]]
    return c


@case
def normal_one_symbol_len1():
    return _one_symbol("normal_one_symbol_len1", 1)


@case
def normal_one_symbol_len8():
    return _one_symbol("normal_one_symbol_len8", 8)


@case
def normal_one_symbol_len15():
    return _one_symbol("normal_one_symbol_len15", 15)


@case
def skewed_green_1_to_15():
    """Lengths 1, 2, ..., 14, 15, 15 on the green alphabet of a 1-bit cache: the three longest codes are literal
    255, length symbol 23 (a copy of 3073 pixels) and the last cache symbol."""
    w, h = 100, 32
    greens = [3 + 17 * i for i in range(13)]
    lengths = {g: i + 1 for i, g in enumerate(greens)}
    lengths.update({255: 14, 256 + 23: 15, 256 + 24 + 1: 15})
    r = rng_of("skewed")
    toks = [("lit", 0xFF000000 | g << 8) for g in greens] + [("lit", 0xFF00FF00)]
    p1 = next(0xFF000000 | g << 8 for g in greens + [255] if cache_slot(0xFF000000 | g << 8, 1) == 1)
    toks += [("lit", p1), ("idx", 1)]
    toks += [("lit", 0xFF000000 | greens[int(r.integers(0, 13))] << 8) for _ in range(w * h - 3073 - len(toks) - 2)]
    toks += [("copy", 3073, 120 + 7), ("lit", 0xFF00FF00), ("idx", 1)]
    codes = [normal(lengths), None, None, None, None]
    return dict(w=w, h=h, image=image(toks, cache_bits=1, codes={0: codes}), tags=["skewed_1_to_15"])


@case
def lengths_8_and_9():
    """All 280 green symbols under the flat code: 232 of 8 bits (in the table), 48 of 9 (behind it)."""
    r = rng_of("l89")
    px = [0xFF000000 | int(g) << 8 for g in list(range(200, 256)) + list(r.integers(0, 256, 40))]
    toks = lits(px) + [("copy", 1 + int(v), 120 + 1 + int(d)) for v, d in zip([0, 1, 2, 3, 4, 6, 8, 12, 16, 24], r.integers(0, 60, 10))]
    n = 96 + sum(t[1] for t in toks[96:])
    w, h = 12, -(-n // 12)
    toks += lits([0xFF000000 | int(g) << 8 for g in r.integers(0, 256, w * h - n)])
    return dict(w=w, h=h, image=image(toks, codes={0: [normal(flat(range(280))), None, None, None, None]}))


# -- code-length codes

@case
def code_length_code_4_lengths():
    return with_code("cl4", 1, normal({3: 1, 200: 1}, ncl=4), need=[3, 200])


@case
def code_length_code_19_lengths():
    lengths = {10 * i: i + 1 for i in range(15)}
    lengths[250] = 15
    return with_code("cl19", 1, normal(lengths, ncl=19), need=[0, 10, 130, 140, 250])


@case
def code_length_code_one_leaf_8():
    return with_code("cl_one_8", 1, normal(ops=[("lit", 8)] * 256, cl={8: 1}), need=[0, 1, 127, 128, 254, 255])


@case
def code_length_code_one_leaf_0():
    return with_code("cl_one_0", 1, normal(ops=[("lit", 0)] * 256, cl={0: 1}), refuse=True)


@case
def code_length_code_incomplete():
    return with_code("cl_inc", 1, normal({3: 1, 200: 1}, cl={0: 2, 1: 2, 18: 2}), need=[3, 200], refuse=True)


@case
def code_length_code_over_subscribed():
    return with_code("cl_over", 1, normal({3: 1, 200: 1}, cl={0: 1, 1: 1, 18: 1}), need=[3, 200], refuse=True)


# -- repeat codes

@case
def repeat_16_first_to_the_end():
    """Nothing but code 16: 8 repeated over all 256 symbols (a code-length code of one leaf), the last run ending on
    the alphabet's last symbol."""
    return with_code("r16f", 2, normal(ops=[(16, 6)] * 42 + [(16, 4)]), need=[0, 9, 255])


@case
def repeat_16_one_past_the_end():
    return with_code("r16p", 2, normal(ops=[(16, 6)] * 42 + [(16, 5)]), refuse=True)


@case
def repeat_16_after_zeros():
    """2, 0, 0, then 16 x 3: the repeated length is the 2, not the zeros and not the initial 8."""
    ops = [("lit", 2), ("lit", 0), ("lit", 0), (16, 3), (18, 138), (18, 112)]
    return with_code("r16z", 3, normal(ops=ops), need=[0, 3, 4, 5])


@case
def repeat_17_and_18_extremes():
    ops = [("lit", 2), (17, 3), ("lit", 2), (17, 10), ("lit", 2), (18, 11), ("lit", 2), (18, 138), (18, 90)]
    assert sum(1 if o == "lit" else n for o, n in ops) == 256
    return with_code("r1718", 1, normal(ops=ops), need=[0, 4, 15, 27])


@case
def repeat_18_one_past_the_end():
    return with_code("r18p", 1, normal(ops=[("lit", 1), ("lit", 1), (18, 138), (18, 117)]), refuse=True)


# -- max_symbol

@case
def max_symbol_widths_0_to_4():
    """max_symbol = 2 in fields of 2, 4, 6, 8 and 10 bits: symbols 0 and 1 of every alphabet."""
    px = [int(p) for p in rng_of("ms04").integers(0, 2, (W0 * H0, 4)) @ np.array([1 << 24, 1 << 16, 1 << 8, 1])]
    px[:2] = [0, 0x01010101]
    codes = [normal(ops=[("lit", 1)] * 2, max_symbol=(2, k)) for k in range(5)]
    return dict(w=W0, h=H0, image=image(lits(px), codes={0: codes}))


@case
def max_symbol_widths_5_to_7():
    px = [int(p) for p in rng_of("ms57").integers(0, 2, (W0 * H0, 4)) @ np.array([1 << 24, 1 << 16, 1 << 8, 1])]
    px[:2] = [0, 0x01010101]
    codes = [None] + [normal(ops=[("lit", 1)] * 2, max_symbol=(2, k)) for k in (5, 6, 7)] + [None]
    return dict(w=W0, h=H0, image=image(lits(px), codes={0: codes}))


@case
def max_symbol_is_the_alphabet():
    return with_code("msa", 1, normal(ops=[("lit", 8)] * 256, max_symbol=(256, 3)), need=[0, 255, 100])


@case
def max_symbol_one_above_the_alphabet():
    return with_code("msa1", 1, normal(ops=[("lit", 8)] * 256, max_symbol=(257, 3)), refuse=True)


@case
def max_symbol_runs_out():
    return with_code("msr", 1, normal(ops=[("lit", 0), ("lit", 2), (16, 3)], max_symbol=(3, 1)), need=[1, 2, 3, 4])


# -- invalid codes

@case
def code_over_subscribed():
    return with_code("co", 1, normal({0: 1, 1: 1, 2: 1}), need=[0, 1], refuse=True)


@case
def code_incomplete_by_one_leaf_at_15():
    return with_code("ci15", 1, normal({i: i + 1 for i in range(15)}), need=[0, 1], refuse=True)


@case
def code_all_zero():
    return with_code("cz", 1, normal(ops=[(18, 138), (18, 118)]), refuse=True)


# -- copies

def noise(name, n):
    return [int(p) for p in rng_of(name).integers(0, 1 << 32, n, dtype=np.uint64)]


@case
def copy_4096_at_distance_1():
    w, h = 65, 64
    toks = lits(noise("c4096", 1)) + [("copy", 4096, 121)] + lits(pixels("c4096", w * h - 4097))
    return dict(w=w, h=h, image=image(toks))


@case
def copy_across_row_ends_overlapping():
    w, h = 7, 6
    toks = lits(pixels("crow", 5, (5, 1, 1, 1))) + [("copy", 20, 122)] + lits(pixels("crow2", 3)) + [("copy", 14, 120 + 9)]
    return dict(w=w, h=h, image=image(toks))


@case
def copy_across_a_tile():
    """9 x 2 under 4-pixel tiles of groups 0, 1, 0: a copy from x = 2 ends at x = 5, inside group 1's tile, whose
    codes the next literal must be read with."""
    a, bb = pixels("ctile_a", 9, (3, 2, 1, 1)), pixels("ctile_b", 9, (3, 2, 2, 1))
    toks = lits(a[:2]) + [("copy", 4, 121)] + lits(bb[:2]) + lits(a[2:3]) + lits(a[3:6]) + [("copy", 5, 120 + 9)] + lits(a[6:7])
    return dict(w=9, h=2, image=image(toks, meta=(2, [[0, 1, 0]])))


@case
def copy_ends_on_the_last_pixel():
    return dict(w=6, h=3, image=image(lits(pixels("clast", 8)) + [("copy", 10, 120 + 8)]))


@case
def copy_one_too_long():
    return dict(w=6, h=3, image=image(lits(pixels("clast", 8)) + [("copy", 11, 120 + 8)]), refuse=True)


@case
def copy_distance_one_beyond_the_start():
    return dict(w=6, h=3, image=image(lits(pixels("clast", 8)) + [("copy", 4, 120 + 9)] + lits(pixels("cd", 6))), refuse=True)


@case
def copy_as_first_token():
    return dict(w=6, h=3, image=image([("copy", 4, 121)] + lits(pixels("cf", 14))), refuse=True)


def _plane_codes(w):
    """9 + 7 w literal pixels of noise (the largest distance is 8 + 7 w), then one copy per plane code 1..120 in a
    seeded order, of 1 or 2 pixels, a literal after every third."""
    name = f"plane{w}"
    r = rng_of(name)
    toks = lits([0xFF000000 | p & 0xFFFFFF for p in noise(name, 9 + 7 * w)])
    for i, c in enumerate(r.permutation(120)):
        toks.append(("copy", 1 + int(r.integers(0, 2)), int(c) + 1))
        if i % 3 == 2:
            toks += lits([0xFF000000 | p & 0xFFFFFF for p in noise(f"{name}/{c}", 1)])
    n = sum(1 if t[0] == "lit" else t[1] for t in toks)
    h = -(-n // w)
    toks += lits([0xFF000000 | p & 0xFF for p in noise(name + "/fill", w * h - n)])
    return dict(w=w, h=h, image=image(toks))


for _w in (1, 2, 8, 9, 17):
    CASES[f"plane_codes_width_{_w}"] = functools.partial(_plane_codes, _w)


def _far(dsym_distance, refuse=None):
    """256 x 256: 300 pixels of noise, copies of 4096 at distance 300 up to pixel 65417, then the copy under test."""
    w = h = 256
    toks = lits([0xFF000000 | p & 0xFFFFFF for p in noise("far", 300)])
    n = 300
    while n + 4096 <= 65417:
        toks.append(("copy", 4096, 120 + 300))
        n += 4096
    toks.append(("copy", 65417 - n, 120 + 300))
    toks.append(("copy", 7, 120 + dsym_distance))
    n = 65417 + 7
    toks.append(("copy", w * h - n, 120 + 299))
    return dict(w=w, h=h, image=image(toks), **({"refuse": True} if refuse else {}))


@case
def distance_symbol_32():
    """Symbol 32 starts at distance code 65537 = distance 65417: the largest symbol whose smallest distance fits
    below 300 x 300 (symbol 33 starts at 98185)."""
    assert prefix_symbol(120 + 65417) == (32, 15, 0)
    return _far(65417)


@case
def distance_symbol_39_beyond_the_start():
    assert prefix_symbol(120 + 786313)[0] == 39
    return _far(786313, refuse=True)


# -- the colour cache

def _cache(bits):
    """Literals that fill some slots, among them the last; hits on the last index, on a slot never written (reads 0)
    and on a pixel that only a copy put back after a colliding literal took its slot."""
    size = 1 << bits
    by_slot = {}
    for k in range(1, 200000):
        p = (0xFF000000 | k * 2654435) & 0xFFFFFFFF
        by_slot.setdefault(cache_slot(p, bits), []).append(p)
        if by_slot.get(size - 1) and len(by_slot.get(0, ())) >= 2:
            break
    last = by_slot[size - 1][0]
    a, c = by_slot[0][0], by_slot[0][1]  # two colours of slot 0
    free = next(s for s in range(size - 1, -1, -1) if s not in (0, size - 1) and s != cache_slot(0, bits)) if size > 2 else None
    toks = [("lit", a), ("lit", last), ("idx", size - 1), ("lit", c), ("idx", 0), ("copy", 1, 120 + 5), ("idx", 0)]
    if free is not None:
        toks += [("idx", free)]
    toks += [("lit", last), ("idx", 0)]
    n = sum(1 if t[0] != "copy" else t[1] for t in toks)
    assert n <= 12
    toks += [("idx", size - 1)] * (12 - n)
    return dict(w=4, h=3, image=image(toks, cache_bits=bits))


for _b in range(1, 12):
    CASES[f"cache_bits_{_b}"] = functools.partial(_cache, _b)


@case
def cache_flag_with_0_bits():
    return dict(w=4, h=3, image=image(lits(pixels("c0", 12)), cache_raw=(1, 0)), refuse=True)


@case
def cache_12_bits():
    return dict(w=4, h=3, image=image(lits(pixels("c12", 12)), cache_raw=(1, 12)), refuse=True)


# -- the entropy image

def _grouped(name, w, h, bits, gmap, **kw):
    """Literals and short copies whose colours depend on the group, so that a token read under another group's
    codes cannot come out right."""
    r = rng_of(name)
    pal = {g: pixels(f"{name}/{g}", 4, (3, 2, 2, 1)) for g in sorted({g for row in gmap for g in row})}
    toks, n = [], 0
    while n < w * h:
        g = gmap[(n // w) >> bits][(n % w) >> bits]
        if n > w and r.integers(0, 4) == 0 and w * h - n > 3:
            toks.append(("copy", int(r.integers(1, 4)), 120 + int(r.integers(1, w))))
            n += toks[-1][1]
        else:
            toks.append(("lit", pal[g][int(r.integers(0, 4))]))
            n += 1
    return dict(w=w, h=h, image=image(toks, meta=(bits, gmap), **kw))


@case
def meta_bits_2_odd_width():
    return _grouped("m2", 11, 6, 2, [[0, 1, 2], [2, 0, 1]])


@case
def meta_bits_9():
    return _grouped("m9", 5, 3, 9, [[1]])  # (one tile; group 0 is in the stream and unused)


@case
def meta_groups_0_and_5():
    return _grouped("m05", 9, 5, 2, [[0, 5, 0], [5, 0, 5]])


@case
def meta_invalid_code_in_an_unused_group():
    c = _grouped("m05", 9, 5, 2, [[0, 5, 0], [5, 0, 5]])
    c["image"]["codes"] = {2: [None, normal({0: 1, 1: 1, 2: 1}), None, None, None]}
    c["refuse"] = "libwebp decides"
    return c


@case
def meta_group_300():
    return _grouped("m300", 6, 2, 2, [[0, 300]])


@case
def meta_invalid_code_in_an_unused_group_of_301():
    c = _grouped("m300", 6, 2, 2, [[0, 300]])
    c["image"]["codes"] = {150: [None, None, None, normal({i: i + 1 for i in range(15)}), None]}
    c["refuse"] = "libwebp decides"
    return c


# -- transforms

def _sub(name, w, h, bits):
    r = (1 << bits) - 1
    return rng_of(name).integers(0, 1 << 32, ((h + r) >> bits, (w + r) >> bits), dtype=np.uint64).astype(np.uint32)


def _residual(name, n):
    return pixels(name, n, (5, 4, 4, 3))


def _pred_data(name, w, h, bits, modes=None):
    d = _sub(name, w, h, bits)
    m = rng_of(name + "/m").integers(1, 14, d.shape).astype(np.uint32) if modes is None else np.asarray(modes, np.uint32).reshape(d.shape)
    return (d & np.uint32(0xFFFF00FF)) | m << 8


def _transformed(name, w, h, order, bits=2, ncolors=5):
    trs, xs = [], w
    r = rng_of(name)
    for t in order:
        if t == P:
            trs.append({"type": P, "bits": bits, "data": _pred_data(f"{name}/p", xs, h, bits)})
        elif t == CC:
            trs.append({"type": CC, "bits": bits, "data": _sub(f"{name}/c", xs, h, bits)})
        elif t == SG:
            trs.append({"type": SG})
        else:
            trs.append({"type": CI, "table": noise(f"{name}/t", ncolors)})
            pk = pack_bits(ncolors)
            xs = (xs + (1 << pk) - 1) >> pk
    if CI in order:
        # the green byte holds the packed indices; what is read after colour indexing works on it at the packed width
        px = [(p & 0xFFFF00FF) | int(g) << 8 for p, g in zip(_residual(name, xs * h), r.integers(0, 256, xs * h))]
    else:
        px = _residual(name, xs * h)
    return dict(w=w, h=h, transforms=trs, image=image(lits(px)))


for _b in range(2, 10):
    CASES[f"predictor_bits_{_b}"] = functools.partial(_transformed, f"pb{_b}", 11, 7, [P], _b)
    CASES[f"cross_color_bits_{_b}"] = functools.partial(_transformed, f"cb{_b}", 11, 7, [CC], _b)
CASES["predictor_on_1x1"] = functools.partial(_transformed, "p11", 1, 1, [P], 9)
CASES["cross_color_on_1x1"] = functools.partial(_transformed, "c11", 1, 1, [CC], 2)


@case
def predictor_all_modes_with_junk():
    """32 x 8 under 4-pixel blocks: sixteen blocks, one per mode 0..15, the other bytes of the mode image random."""
    w, h = 32, 8
    modes = rng_of("pm").permutation(16).reshape(2, 8)
    return dict(w=w, h=h, transforms=[{"type": P, "bits": 2, "data": _pred_data("pm", w, h, 2, modes)}],
                image=image(lits(noise("pm/res", w * h))))


def orders():
    """ORDERS of tests/test_gpu_lossless.py: every order of the four transforms the kernel's tests run."""
    import ast
    src = (ROOT / "tests" / "test_gpu_lossless.py").read_text()
    node = next(n for n in ast.parse(src).body if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") == "ORDERS")
    names = {"P": P, "CC": CC, "SG": SG, "CI": CI}
    return [[names[e.id] for e in lst.elts] for lst in node.value.elts]


for _o in orders():
    _n = "order_" + "_".join(("p", "cc", "sg", "ci")[t] for t in _o)
    CASES[_n] = functools.partial(_transformed, _n, 10, 6, _o, 2, (2, 4, 11, 40)[len(CASES) % 4])


@case
def transform_repeated():
    return dict(w=4, h=3, transforms=[{"type": SG}, {"type": SG}], image=image(lits(pixels("tr", 12))), refuse=True)


def _indexed(ncolors, w):
    """Colour indexing alone, h = 3: indices over the whole range the packing can hold, so that tables the packing
    is wider than are read beyond their end."""
    name = f"ci{ncolors}w{w}"
    pk = pack_bits(ncolors)
    top = min(1 << (8 >> pk), ncolors + 3)
    idx = rng_of(name).integers(0, top, (3, w))
    idx[0, 0] = top - 1
    xs = (w + (1 << pk) - 1) >> pk
    px = []
    for y in range(3):
        for x in range(xs):
            g = 0
            for k in range(1 << pk):
                if (x << pk) + k < w:
                    g |= int(idx[y, (x << pk) + k]) << (k * (8 >> pk))
            px.append(0xFF000000 | g << 8 | (x * 5 + y) << 16 & 0xFF0000)
    return dict(w=w, h=3, transforms=[{"type": CI, "table": noise(name, ncolors)}], image=image(lits(px)))


for _nc in (1, 2, 3, 4, 5, 16, 17, 256):
    for _w in (1, 7, 8, 9):
        CASES[f"color_index_{_nc}_colors_width_{_w}"] = functools.partial(_indexed, _nc, _w)


# -- ALPH

def _alph_tokens(name, junk=True):
    r = rng_of(name)
    n = ALPH_W * ALPH_H
    greens = r.choice(256, size=9, replace=False)
    toks, k = [], 0
    while k < n:
        if k > 8 + 7 * ALPH_W and r.integers(0, 3) == 0:
            ln = min(int(r.integers(1, 40)), n - k)
            toks.append(("copy", ln, int(r.integers(1, 121)) if r.integers(0, 2) else 120 + int(r.integers(1, k))))
            k += ln
        else:
            p = int(greens[r.integers(0, 9)]) << 8
            if junk:
                p |= int(r.integers(0, 3)) << 24 | int(r.integers(0, 3)) << 16 | int(r.integers(0, 3))
            toks.append(("lit", p))
            k += 1
    return toks


def _alph(flt):
    name = f"alph{flt}"
    return dict(w=ALPH_W, h=ALPH_H, container="alph", filter=flt, image=image(_alph_tokens(name), cache_bits=3 if flt & 1 else 0))


for _f in range(4):
    CASES[f"alph_filter_{_f}"] = functools.partial(_alph, _f)


@case
def alph_color_index():
    table = [int(v) << 8 | (0xFF0000FF if i & 1 else 0) for i, v in enumerate((0, 255, 96, 200))]
    xs = (ALPH_W + 3) >> 2
    px = [int(g) << 8 for g in rng_of("alph_ci").integers(0, 256, xs * ALPH_H)]
    return dict(w=ALPH_W, h=ALPH_H, container="alph", filter=1, transforms=[{"type": CI, "table": table}], image=image(lits(px)))


@case
def alph_predictor():
    return dict(w=ALPH_W, h=ALPH_H, container="alph", filter=2,
                transforms=[{"type": P, "bits": 4, "data": _pred_data("alph_p", ALPH_W, ALPH_H, 4)}], image=image(_alph_tokens("alph_p")))


# -- containers

@case
def container_vp8x():
    gmap = rng_of("cx/map").integers(0, 4, (6, 9)).tolist()  # 67 x 45, the size of the lossy fixtures, under 8-pixel tiles
    c = _grouped("cx", 67, 45, 3, gmap)
    c["container"] = "vp8x"
    return c


NAMES = tuple(CASES)


# ---- what the cases must reach (the issue's list), as features the writer records while it writes -----------------

def required():
    req = {"pixel_data_of_zero_bits", "stream_ends_on_the_group_bound", "simple_one_1bit", "simple_one_8bit", "simple_two_8bit_first",
           "simple_two_1bit_first", "simple_same_symbol", "lengths_8_and_9", "skewed_1_to_15", "repeat_16_first",
           "repeat_16_after_zeros", "run_ends_at_alphabet_end", "max_symbol_2", "max_symbol_alphabet", "max_symbol_runs_out",
           "longest_length_symbol", "copy_overlaps", "copy_crosses_several_row_ends", "copy_crosses_tile", "copy_ends_on_last_pixel",
           "cache_slot_never_written", "cache_hit_entered_by_copy", ("cache_collision", 1), "meta_width_not_multiple_of_tile",
           "group_changes_mid_row", "group_above_255", "mode_image_junk", "index_beyond_table", "table_deltas_wrap",
           "alph_junk_in_other_channels", ("unused_groups", 4), ("meta_bits", 2), ("meta_bits", 9), ("distance_symbol", 32),
           ("plane_code_clamped", "zero"), ("plane_code_clamped", "negative"), ("code_length_lengths", 4), ("code_length_lengths", 19),
           ("code_length_code_one_leaf", 8), ("repeat_17", 3), ("repeat_17", 10), ("repeat_18", 11), ("repeat_18", 138),
           ("container", "riff"), ("container", "vp8x"), ("container", "alph"), ("alph_transform", CI), ("alph_transform", P),
           ("transform_on_1x1", P), ("transform_on_1x1", CC)}
    req |= {("simple_top_symbol", f"main:{c}") for c in "grbad"}
    req |= {("normal_one_symbol", l) for l in (1, 8, 15)}
    req |= {("code_longer_than_8", l) for l in range(9, 16)}
    req |= {("max_symbol_width", k) for k in range(8)}
    req |= {("plane_code", w, c) for w in (1, 2, 8, 9, 17) for c in range(1, 121)}
    req |= {("cache_bits", b) for b in range(1, 12)} | {("cache_last_index", b) for b in range(1, 12)}
    req |= {("predictor_bits", b) for b in range(2, 10)} | {("cross_color_bits", b) for b in range(2, 10)}
    req |= {("predictor_mode", m) for m in range(16)}
    req |= {("order", tuple(o)) for o in orders()}
    req |= {("color_index_colors", n) for n in (1, 2, 3, 4, 5, 16, 17, 256)} | {("color_index_width", w) for w in (1, 7, 8, 9)}
    req |= {("alph_filter", f) for f in range(4)}
    return req


REFUSALS = ("zero_bits_two_groups_one_short", "simple_distance_40", "code_length_code_one_leaf_0", "code_length_code_incomplete",
            "code_length_code_over_subscribed", "repeat_16_one_past_the_end", "repeat_18_one_past_the_end",
            "max_symbol_one_above_the_alphabet", "code_over_subscribed", "code_incomplete_by_one_leaf_at_15", "code_all_zero",
            "copy_one_too_long", "copy_distance_one_beyond_the_start", "copy_as_first_token", "distance_symbol_39_beyond_the_start",
            "cache_flag_with_0_bits", "cache_12_bits", "transform_repeated")
