"""A test-only FLAC writer (RFC 9639).  It is not an optimiser: it writes what it is told to write -- per frame the blocking strategy, the
block size and the form of its code, the form of the rate code, the channel assignment and the sample-size code; per subframe the type
(CONSTANT / VERBATIM / FIXED order / LPC with given coefficients, precision and shift), the wasted bits, the residual method, the partition
order and per partition the Rice parameter or the escape width; and the MD5.  Plain Python integers; `lpc_residuals` is the one piece of
arithmetic, and tests pin it against numpy.diff."""
from __future__ import annotations

import hashlib

import numpy as np

from tts_indic_server_f5_amd import wave_codec as W

BLOCK_CODES = {192: 1, 576: 2, 1152: 3, 2304: 4, 4608: 5, **{256 << c: 8 + c for c in range(8)}}
RATE_CODES = {88200: 1, 176400: 2, 192000: 3, 8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10, 96000: 11}
SIZE_CODES = {8: 1, 12: 2, 16: 4, 20: 5, 24: 6, 32: 7}
FIXED = W._FLAC_FIXED


class Bits:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, value, bits):
        if bits:
            self.v = (self.v << bits) | (int(value) & ((1 << bits) - 1))
            self.n += bits

    def unary(self, zeros):
        self.v = (self.v << (zeros + 1)) | 1
        self.n += zeros + 1

    def bytes(self):
        pad = -self.n % 8
        return ((self.v << pad).to_bytes((self.n + pad) // 8, "big")) if self.n else b""


def sub(kind="verbatim", order=0, coefs=None, precision=None, shift=0, wasted=0, method=0, porder=0, params=None, residuals=None):
    """A subframe spec.  kind: "constant", "verbatim", "fixed" (order 0..4) or "lpc" (coefs, precision, shift).  params: per partition a Rice
    parameter k or ("esc", width); None: the smallest k whose codes average under two unary zeros.  residuals: written instead of the
    predictor's own (the samples then only give the warm-up), for streams that decode to something else than they were made from."""
    return dict(kind=kind, order=len(coefs) if coefs is not None else order, coefs=coefs, precision=precision, shift=shift, wasted=wasted,
                method=method, porder=porder, params=params, residuals=residuals)


def lpc_residuals(x, coefs, shift):
    """res[i] = x[i] - (sum(coefs[j] * x[i-1-j]) >> shift) for i >= len(coefs), in Python integers."""
    x, o = [int(v) for v in x], len(coefs)
    return [x[i] - (sum(c * x[i - 1 - j] for j, c in enumerate(coefs)) >> shift) for i in range(o, len(x))]


def _fits(v, bits):
    return bits > 0 and -(1 << (bits - 1)) <= v <= (1 << (bits - 1)) - 1


def _put_residual(w, res, b, o, method, porder, params):
    pbits = 4 + method
    w.put(method, 2)
    w.put(porder, 4)
    parts = 1 << porder
    assert b % parts == 0 and b >> porder >= o, (b, porder, o)
    params = list(params) if isinstance(params, (list, tuple)) and not (len(params) == 2 and params[0] == "esc") else [params] * parts
    assert len(params) == parts
    at = 0
    for p in range(parts):
        n = (b >> porder) - (o if p == 0 else 0)
        r = res[at:at + n]
        at += n
        u = [2 * v if v >= 0 else -2 * v - 1 for v in r]
        k = params[p]
        if k is None:
            mean = sum(u) // max(len(u), 1)
            k = min(max(mean.bit_length() - 1, 0), (1 << pbits) - 2)
        if isinstance(k, tuple):
            width = k[1]
            assert all(v == 0 if width == 0 else _fits(v, width) for v in r), ("escape width", width)
            w.put((1 << pbits) - 1, pbits)
            w.put(width, 5)
            for v in r:
                w.put(v, width)
        else:
            assert 0 <= k < (1 << pbits) - 1
            w.put(k, pbits)
            for v in u:
                w.unary(v >> k)
                w.put(v, k)


def _put_subframe(w, x, depth, s):
    x, b, wasted = [int(v) for v in x], len(x), s["wasted"]
    if wasted:
        assert all(v % (1 << wasted) == 0 for v in x), "wasted bits need multiples of 2**wasted"
        x = [v >> wasted for v in x]
    depth -= wasted
    kind, o = s["kind"], s["order"]
    assert all(_fits(v, depth) for v in (x[:o] if s["residuals"] is not None else x)), ("samples outside", depth)
    code = {"constant": 0, "verbatim": 1, "fixed": 8 + o, "lpc": 31 + o}[kind]
    w.put(0, 1)
    w.put(code, 6)
    w.put(1 if wasted else 0, 1)
    if wasted:
        w.unary(wasted - 1)
    if kind == "constant":
        assert len(set(x)) == 1
        w.put(x[0], depth)
    elif kind == "verbatim":
        for v in x:
            w.put(v, depth)
    else:
        coefs, shift = (FIXED[o], 0) if kind == "fixed" else (tuple(s["coefs"]), s["shift"])
        for v in x[:o]:
            w.put(v, depth)
        if kind == "lpc":
            precision = s["precision"]
            assert 1 <= precision <= 15 and all(_fits(c, precision) for c in coefs) and 0 <= shift <= 15
            w.put(precision - 1, 4)
            w.put(shift, 5)
            for c in coefs:
                w.put(c, precision)
        _put_residual(w, lpc_residuals(x, coefs, shift) if s["residuals"] is None else [int(v) for v in s["residuals"]], b, o, s["method"], s["porder"], s["params"])


def frame(planes, number, rate, bits, subs, stereo=None, variable=False, block_form="auto", rate_form="table", size_form="code", coded=False):
    """One frame of `planes` (a list of channels, equal lengths) as frame / sample `number`.  stereo: None (independent channels) or the channel
    code 8 left/side, 9 side/right, 10 mid/side.  block_form: "auto" (the table code when there is one, else the shorter of the two
    explicit forms), "8" or "16"; rate_form: "info", "table", "khz", "hz" or "dahz"; size_form: "code" or "info"; coded: the planes are the
    coded pair already (left/side, side/right, mid/side), written as they are."""
    planes = [[int(v) for v in p] for p in planes]
    b, ch = len(planes[0]), len(planes)
    if stereo is not None and not coded:
        left, right = planes
        side = [l - r for l, r in zip(left, right)]
        planes = {8: [left, side], 9: [side, right], 10: [[(l + r) >> 1 for l, r in zip(left, right)], side]}[stereo]
    ch_code = ch - 1 if stereo is None else stereo
    if block_form == "auto":
        block_form = "table" if b in BLOCK_CODES else "8" if b <= 256 else "16"
    bs_code = BLOCK_CODES[b] if block_form == "table" else 6 if block_form == "8" else 7
    rate_code = {"info": 0, "khz": 12, "hz": 13, "dahz": 14}.get(rate_form) if rate_form != "table" else RATE_CODES[rate]
    head = bytes([0xFF, 0xF8 | int(variable), (bs_code << 4) | rate_code, (ch_code << 4) | ((SIZE_CODES[bits] if size_form == "code" else 0) << 1)])
    head += W._flac_number(number)
    if bs_code in (6, 7):
        head += (b - 1).to_bytes(bs_code - 5, "big")
    if rate_code == 12:
        assert rate % 1000 == 0
        head += bytes([rate // 1000])
    elif rate_code == 13:
        head += rate.to_bytes(2, "big")
    elif rate_code == 14:
        assert rate % 10 == 0
        head += (rate // 10).to_bytes(2, "big")
    head += bytes([W.flac_crc8(head)])
    w = Bits()
    for c, (p, s) in enumerate(zip(planes, subs)):
        side = stereo is not None and ((stereo in (8, 10) and c == 1) or (stereo == 9 and c == 0))
        _put_subframe(w, p, bits + side, s)
    body = head + w.bytes()
    return body + W.flac_crc16(body).to_bytes(2, "big")


def md5_of(x, bits):
    width = (bits + 7) // 8
    x = np.asarray(x, dtype=np.int64)
    return hashlib.md5(b"".join(int(v).to_bytes(width, "little", signed=True) for v in x.T.reshape(-1))).digest()


def stream_header(rate, channels, bits, total, md5=bytes(16), min_block=16, max_block=65535, extra_blocks=(), min_frame=0, max_frame=0):
    """ "fLaC", STREAMINFO and `extra_blocks` ((type, payload) pairs) behind it."""
    info = (min_block.to_bytes(2, "big") + max_block.to_bytes(2, "big") + min_frame.to_bytes(3, "big") + max_frame.to_bytes(3, "big")
            + ((rate << 44) | ((channels - 1) << 41) | ((bits - 1) << 36) | total).to_bytes(8, "big") + md5)
    blocks = [(0, info)] + list(extra_blocks)
    out = b"fLaC"
    for i, (kind, payload) in enumerate(blocks):
        out += bytes([kind | (0x80 if i == len(blocks) - 1 else 0)]) + len(payload).to_bytes(3, "big") + payload
    return out


def write_flac(x, rate, bits, block=4096, subs=None, stereo=None, variable=False, md5=True, extra_blocks=(), total=None, blocks=None,
               min_block=None, max_block=None, **forms):
    """A whole stream of x (int [channels, n] or [n]).  `blocks`: the block sizes, default `block` repeated with a short last one; `subs`: one
    spec per channel, or a function (frame index, channel) -> spec; `stereo`: a channel code for every frame or a function of the frame
    index; `md5`: True (computed), False (zero) or 16 bytes; `forms`: `frame`'s block_form / rate_form / size_form."""
    x = np.atleast_2d(np.asarray(x, dtype=np.int64))
    ch, n = x.shape
    if blocks is None:
        blocks = [block] * (n // block) + ([n % block] if n % block else [])
    assert sum(blocks) == n
    frames, at = [], 0
    for i, b in enumerate(blocks):
        s = [subs(i, c) for c in range(ch)] if callable(subs) else list(subs) if subs is not None else [sub()] * ch
        st = stereo(i) if callable(stereo) else stereo
        frames.append(frame([x[c, at:at + b] for c in range(ch)], at if variable else i, rate, bits, s, st, variable, **forms))
        at += b
    digest = md5_of(x, bits) if md5 is True else bytes(16) if md5 is False else md5
    sizes = [len(f) for f in frames] or [0]
    head = stream_header(rate, ch, bits, n if total is None else total, digest, min(blocks) if min_block is None and blocks else (min_block or 16),
                         max(blocks) if max_block is None and blocks else (max_block or 16), extra_blocks, min(sizes), max(sizes))
    return head + b"".join(frames), [len(head)] + [len(f) for f in frames]
