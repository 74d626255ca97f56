"""IQ recordings synthesised to reproduce the reference's two UAT 978 golden callback texts, line by line (the 978 counterpart of
golden_text.py).

The reference keeps the text its test printed for two 978 captures (tests/golden/reference/TestEnv_rtlsdr_978_*.txt(.gz)); the
captures are not in the snapshot.  For every line this module builds ONE downlink frame that makes the wrapper's rules
(uat2json-wrapper.cpp:18-121 over dump978's MDB decoder; tests/uat_mdb.py) print exactly that line after the frame: a short type-0
state-vector frame with the line's position, altitude and speed (north/south velocity = speed, east/west 0), or, where the line shows
a call sign its address has not had before, a long type-1 frame carrying the same state vector and the call sign with CSID set.  Later
lines of that address keep printing the call sign from the tracker's state alone (the sticky rule).  A line that repeats its
predecessor gets the identical frame again.  The frames are Reed-Solomon encoded (oracle_py.rs_parity978) and modulated into u8 IQ: the phase
moves +-0.3 pi per sample, I,Q on a circle around 127.5 (the centre of the reference LUT, UAT978.cpp:76-100), noise around 127.

Where a frame may sit: UAT978Handler::HandleData (UAT978.cpp:43-60) stages 65 536 phases at a time and carries only half of the
unconsumed tail (it passes the entry count as memmove's byte count), so some stretches of the stream are never examined and some
stage positions are examined twice.  `zones` follows that staging for a given call size and returns the stream intervals in which a
frame is reported exactly once; frames are placed only where that holds for the whole stream in one call, for 262 144-byte calls and
for one process_buffer over the stream.  What this pins: the MDB field decoders, the sticky-state rules and the formatter, tied to
reference-held text.  It is not parity with a capture: the inputs are chosen.
"""
import gzip
import math
import os

import numpy as np

import golden_text as G
import uat_helpers as U

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE_TEXT = {
    "short": os.path.join(HERE, "golden", "reference", "TestEnv_rtlsdr_978_2021-06-16-20-21-39.txt"),
    "long": os.path.join(HERE, "golden", "reference", "TestEnv_rtlsdr_978_2021-06-16-22-30-43.txt.gz"),
}
STAGE = 65536                  # phases per staging round (UAT978.cpp:48)
MAX_FRAME_BITS = 36 + 4416     # the scan loop stops this many bits before a buffer's end
CALL_BYTES = 262144            # RTLSDR::BufferLength: one HandleData call of the live path
MARGIN = 128                   # samples kept clear around each frame
BASE40 = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ  .."


def read_lines(name):
    path = REFERENCE_TEXT[name]
    op = gzip.open if path.endswith(".gz") else open
    with op(path, "rt", encoding="latin-1", newline="\n") as f:
        return f.read().splitlines()


def parse(name):
    out = []
    for ln in read_lines(name):
        m = G.LINE.match(ln)
        assert m, ln
        out.append(dict(text=ln, addr=int(m.group(1), 16), callsign=m.group(2), lat=m.group(3), lon=m.group(4),
                        altitude=int(m.group(5)), speed=int(m.group(6)), squawk=int(m.group(7))))
    return out


def _raw_angle(text, full, wrap):
    """The raw 23/24-bit angle whose decoded value prints as `text` ("%+03.2f" of the truncated 1e-7 degrees)."""
    deg = float(text)
    raw = int(round((deg + wrap if deg < 0 else deg) / 360.0 * (1 << 24)))
    for d in sorted(range(-64, 65), key=abs):
        r = raw + d
        if not 0 <= r < full:
            continue
        v = r * 360.0 / 16777216.0
        if v > wrap / 2:
            v -= wrap
        if "%+03.2f" % (int(v * 10000000) / 10000000.0) == text:
            return r
    raise AssertionError("no raw angle prints as " + text)


def payload_for(ln, with_callsign=True):
    """The frame payload for one golden line: 34 bytes, type 1 with the line's call sign, when the line shows one and
    `with_callsign`; 18 bytes, type 0, otherwise."""
    assert ln["squawk"] == 0
    cs = ln["callsign"]
    long_ = with_callsign and cs != "\0" * 8
    f = bytearray(34 if long_ else 18)
    f[0] = (1 if long_ else 0) << 3
    f[1:4] = ln["addr"].to_bytes(3, "big")
    raw_lat = _raw_angle(ln["lat"], 1 << 23, 180)
    raw_lon = _raw_angle(ln["lon"], 1 << 24, 360)
    f[4], f[5] = raw_lat >> 15, (raw_lat >> 7) & 0xFF
    f[6] = ((raw_lat & 0x7F) << 1) | (raw_lon >> 23)
    f[7], f[8], f[9] = (raw_lon >> 15) & 0xFF, (raw_lon >> 7) & 0xFF, (raw_lon & 0x7F) << 1
    alt = ln["altitude"]
    assert (alt + 1000) % 25 == 0
    raw_alt = (alt + 1000) // 25 + 1
    assert 0 < raw_alt < 4096
    nic = 8  # position valid whatever the raw angles are
    f[10], f[11] = raw_alt >> 4, ((raw_alt & 15) << 4) | nic
    speed = ln["speed"]
    assert 0 <= speed < 1023
    raw_ns, raw_ew = speed + 1, 1  # airborne subsonic (ag = 0): north speed kt, east 0 kt
    f[12] = raw_ns >> 6
    f[13] = ((raw_ns & 0x3F) << 2) | (raw_ew >> 9)
    f[14] = (raw_ew >> 1) & 0xFF
    f[15] = (raw_ew & 1) << 7  # vertical rate: not available
    if long_:
        chars = cs.replace("\0", " ")
        assert cs.rstrip("\0") == chars.rstrip(" ") and chars[0] != " ", repr(cs)
        idx = [BASE40.index(c) for c in chars]
        words = [idx[0] * 40 + idx[1], idx[2] * 1600 + idx[3] * 40 + idx[4], idx[5] * 1600 + idx[6] * 40 + idx[7]]  # emitter category 0
        for w, v in enumerate(words):
            f[17 + 2 * w], f[18 + 2 * w] = v >> 8, v & 0xFF
        f[26] = 0x02  # CSID: the characters are a call sign
    return bytes(f)


def rounds(nsamples, call_samples):
    """The process_buffer calls HandleData makes over a stream fed in calls of `call_samples` samples, with the reference's half-tail
    carry, assuming no frame runs past a call's last examined bit: [(fresh stage position, fresh stream sample, count, buffer length)]."""
    out, used, start = [], 0, 0
    while start < nsamples:
        n, j = min(call_samples, nsamples - start), 0
        while j < n:
            take = min(STAGE - used, n - j)
            i = used + take
            out.append((used, start + j, take, i))
            j += take
            lenbits = i // 2 - MAX_FRAME_BITS
            done = max(0, (lenbits - 18) * 2) if lenbits > 0 else 0
            used = i - done if done else i
        start += n
    return out


def zones(nsamples, call_samples):
    """Stream intervals [lo, hi) in which a frame is reported exactly once (see the module docstring)."""
    z = []
    for fresh_at, stream_at, take, i in rounds(nsamples, call_samples):
        lenbits = i // 2 - MAX_FRAME_BITS
        if lenbits <= 18:
            continue
        done = (lenbits - 18) * 2
        tail = i - done
        lo = max(fresh_at, tail, 2 * 19) + MARGIN   # past the stage positions the next round re-reads as stale entries
        hi = min(fresh_at + take, done) - MARGIN    # the frame ends before the samples carried to the next round
        if hi > lo:
            z.append((stream_at + lo - fresh_at, stream_at + hi - fresh_at))
    return z


def _intersect(a, b):
    out, i, j = [], 0, 0
    while i < len(a) and j < len(b):
        lo, hi = max(a[i][0], b[j][0]), min(a[i][1], b[j][1])
        if lo < hi:
            out.append((lo, hi))
        if a[i][1] < b[j][1]:
            i += 1
        else:
            j += 1
    return out


def place(lengths, nsamples):
    """Start samples for frames of the given lengths, or None when the stream is too short."""
    whole = [(2 * 19 + MARGIN, 2 * (nsamples // 2 - MAX_FRAME_BITS - 18) - MARGIN)]  # one process_buffer over the stream
    ok = _intersect(_intersect(zones(nsamples, nsamples), zones(nsamples, CALL_BYTES // 2)), whole)
    starts, z, at = [], 0, None
    for L in lengths:
        while z < len(ok):
            lo, hi = ok[z]
            at = lo if at is None or at < lo else at
            if at + L <= hi:
                break
            z, at = z + 1, None
        if z == len(ok):
            return None
        starts.append(at)
        at += L + MARGIN
    return starts


def modulate(codewords, starts, nsamples, amplitude=100.0, noise=2, seed=978):
    """u8 IQ: background noise around 127, each frame (36 sync bits + code word bits) from its start sample.  A 552-byte code word
    (uat_helpers.uplink_frame) is sent behind the uplink sync word, any other behind the ADS-B one."""
    rng = np.random.default_rng(seed)
    iq = (127 + rng.integers(-noise, noise + 1, size=2 * nsamples)).astype(np.int64)
    for cw, at in zip(codewords, starts):
        sync = U.UPLINK_SYNC if len(cw) == 552 else U.ADSB_SYNC
        bits = np.array(U.bits_of(sync, 36) + U.bytes_to_bits(cw), dtype=np.int64)
        steps = np.repeat(np.where(bits > 0, 0.3 * math.pi, -0.3 * math.pi), 2)
        phi = rng.uniform(0, 2 * math.pi) + np.concatenate([[0.0], np.cumsum(steps)])
        s = 2 * at + 2 * np.arange(phi.size)
        iq[s] += np.rint(127.5 + amplitude * np.cos(phi)).astype(np.int64) - 127
        iq[s + 1] += np.rint(127.5 + amplitude * np.sin(phi)).astype(np.int64) - 127
    return np.clip(iq, 0, 255).astype(np.uint8)


def callsign_frames(lines):
    """Which lines carry their call sign: those where it first appears (or changes) for the line's address."""
    shown, out = {}, []
    for ln in lines:
        cs = ln["callsign"]
        have = shown.get(ln["addr"], "\0" * 8)
        assert cs == have or cs != "\0" * 8, "a call sign cannot disappear: " + ln["text"]
        out.append(cs != have)
        shown[ln["addr"]] = cs
    return out


def stream_of(payloads):
    """u8 IQ carrying the payloads (18 / 34 / 432 bytes), RS-encoded, each where it is reported exactly once."""
    coders = {18: U.short_frame, 34: U.long_frame, 432: U.uplink_frame}
    codewords = [coders[len(p)](p) for p in payloads]
    lengths = [2 * (36 + 8 * len(cw)) + 2 for cw in codewords]
    nsamples = 2 * STAGE
    while True:
        starts = place(lengths, nsamples)
        if starts is not None:
            break
        nsamples = int(nsamples * 1.25) // STAGE * STAGE + STAGE
    return modulate(codewords, starts, nsamples)


def build(name):
    """(u8 IQ stream, the payloads in stream order, the expected callback lines) for REFERENCE_TEXT[name]."""
    lines = parse(name)
    payloads = [payload_for(ln, cs) for ln, cs in zip(lines, callsign_frames(lines))]
    return stream_of(payloads), payloads, [ln["text"] for ln in lines]
