"""UAT 978 aircraft tracking without a GPU: the synthesised golden IQ, the test-side restatement (tests/uat_mdb.py) against the
reference's golden text, and the host build of the product's MDB decoder (mdb978.h) against the restatement on exhaustive sets."""
import ctypes as C
import math

import numpy as np
import pytest

import libadsb_amd as A
from oracle import oracle_py as O

import uat_golden_text as UG
import uat_mdb as M

CHUNK = 1 << 20


@pytest.fixture(scope="module", params=["short", "long"])
def golden(request):
    iq, payloads, lines = UG.build(request.param)
    return request.param, iq, payloads, lines


def test_golden_iq_demodulates_to_exactly_the_frames_built(golden):
    _, iq, payloads, _ = golden
    for step in (iq.size, UG.CALL_BYTES):  # HandleData over the whole stream, and in live-sized calls
        o = O.Oracle978()
        got = []
        for k in range(0, iq.size, step):
            got += o.handle_data(iq[k:k + step])
        assert [(ud, p) for ud, p, _, _ in got] == [("-", p) for p in payloads], step
    phi = O.phase_lut978()[iq.view(np.uint16)]
    got, _ = O.process_buffer978(phi)
    assert [p for _, p, _, _ in got] == payloads


def test_restated_tracker_prints_the_golden_text(golden):
    name, iq, payloads, lines = golden
    assert len(lines) == {"short": 42, "long": 9053}[name]
    frames, _ = O.process_buffer978(O.phase_lut978()[iq.view(np.uint16)])
    _, rows = M.Tracker().run(frames)
    assert [M.format_row(r) for r in rows] == lines
    assert any("\0" in ln for ln in lines)  # NUL padding of the call sign is part of the text


# ---- the exhaustive sets (shared with the device test)
def frames_every_type(seed=1, per_type=2000, nbytes=34):
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, size=(32 * per_type, nbytes), dtype=np.uint8)
    f[:, 0] = (np.repeat(np.arange(32), per_type) << 3) | (f[:, 0] & 7)
    return f


def frames_lat(lo, hi):
    raw = np.arange(lo, hi, dtype=np.int64)
    f = np.zeros((raw.size, 12), dtype=np.uint8)
    f[:, 4], f[:, 5], f[:, 6] = raw >> 15, (raw >> 7) & 0xFF, (raw & 0x7F) << 1
    return f


def frames_lon(lo, hi):
    raw = np.arange(lo, hi, dtype=np.int64)
    f = np.zeros((raw.size, 12), dtype=np.uint8)
    f[:, 6], f[:, 7], f[:, 8], f[:, 9] = raw >> 23, (raw >> 15) & 0xFF, (raw >> 7) & 0xFF, (raw & 0x7F) << 1
    return f


def frames_velocity(ag, lo, hi):
    """Raw (ns, ew) pairs k = raw_ns << 11 | raw_ew for k in [lo, hi), air/ground state ag, vertical rate from k as well."""
    k = np.arange(lo, hi, dtype=np.int64)
    raw_a, raw_b = k >> 11, k & 0x7FF
    f = np.zeros((k.size, 17), dtype=np.uint8)
    f[:, 12] = (ag << 6) | (raw_a >> 6)
    f[:, 13] = ((raw_a & 0x3F) << 2) | (raw_b >> 9)
    f[:, 14] = (raw_b >> 1) & 0xFF
    f[:, 15] = ((raw_b & 1) << 7) | ((k >> 4) & 0x7F)
    f[:, 16] = (k & 0xF) << 4
    return f


def frames_uplink(seed=3, count=4000):
    return np.random.default_rng(seed).integers(0, 256, size=(count, 432), dtype=np.uint8)


def exhaustive_sets():
    """(label, frames) pieces of at most CHUNK frames: every type with random bytes, all 2^23 raw latitudes and 2^24 raw longitudes,
    all 2^22 raw (ns, ew) pairs subsonic, supersonic and on the ground (ground: every track code), uplink-sized frames."""
    yield "types", frames_every_type()
    for lo in range(0, 1 << 23, CHUNK):
        yield "lat", frames_lat(lo, lo + CHUNK)
    for lo in range(0, 1 << 24, CHUNK):
        yield "lon", frames_lon(lo, lo + CHUNK)
    for ag in (0, 1, 2):
        for lo in range(0, 1 << 22, CHUNK):
            yield "velocity ag=%d" % ag, frames_velocity(ag, lo, lo + CHUNK)
    yield "uplink", frames_uplink()


def assert_mdb_equal(got, want, label):
    for field in M.MDB_DTYPE.names:
        bad = np.flatnonzero(got[field] != want[field])
        assert bad.size == 0, "%s: %s differs at %d of %d (got %r, want %r)" % (label, field, bad[0], got.size, got[bad[0]], want[bad[0]])


def test_host_decoder_equals_the_restatement_on_exhaustive_sets(native_libs):
    for label, f in exhaustive_sets():
        assert_mdb_equal(A.uat_mdb_decode(f), M.decode_many(f), label)


def test_track_angle_is_never_near_a_whole_degree_off_the_eight_directions():
    """The argument of mdb978.h: for |ns|, |ew| <= 1022 off ns = 0, ew = 0, |ns| = |ew| the track before truncation is at least 1e-6
    degrees from a whole number, far above any double-precision atan2 error; supersonic pairs are the same angles x 4."""
    v = np.arange(-1022, 1023, dtype=np.float64)
    worst = 1.0
    for ns in v:
        ew = v[(v != 0) & (np.abs(v) != abs(ns))]
        if ns == 0:
            continue
        t = 450 - np.arctan2(ns, ew) * 180 / math.pi
        worst = min(worst, float(np.min(np.abs(t - np.rint(t)))))
    assert worst > 1e-6, worst


def test_decoder_fields_by_hand(native_libs):
    """A few values worked out from the published rules (dump978 uat_decode.c) by hand, held against both the restatement and the
    product's decoder (host build)."""
    golden_line = UG.parse("short")[2]  # a6c237[N5344K\0\0]: Pos=+47.57:-122.03^02700 Speed=111
    ground = np.zeros(34, dtype=np.uint8)
    ground[12], ground[13], ground[14] = 0x80, (0x10 << 2) | 0b01, 0x40  # on the ground: raw speed 0x10, track code 1, track bits 0x80
    frames = np.zeros((3, 34), dtype=np.uint8)
    frames[0] = np.frombuffer(UG.payload_for(golden_line), dtype=np.uint8)
    frames[1] = ground
    frames[2, 0] = 0x58  # type 11: header only
    for decoded in (M.decode_many(frames), A.uat_mdb_decode(frames)):
        m, g, h = decoded
        assert m["address"] == 0xA6C237 and m["mdb_type"] == 1 and bytes(m["callsign"]).ljust(8, b"\0") == b"N5344K\0\0"
        assert (m["altitude"], m["speed"], m["track"]) == (2700, 111, 0)
        assert (g["speed"], g["track"], g["valid"] & (M.V_SPEED | M.V_TRACK)) == (15, 90, M.V_SPEED | M.V_TRACK)
        assert h["valid"] == 0


# ---- the sticky rule: one address, frames that leave fields out (shared with the device test)
A1, A2 = 0xABC123, 0x5A5A5A


def sv_payload(addr, mdb_type, raw_lat=0, raw_lon=0, nic=0, raw_alt=0, ag=0, raw_a=0, raw_b=0, raw_v=0, callsign=None, csid=True, size=None):
    """A frame payload with the given raw state-vector fields (0: not available) and, for types 1 / 3, the mode-status call sign."""
    f = bytearray(size or (18 if mdb_type == 0 else 34))
    f[0] = mdb_type << 3
    f[1:4] = addr.to_bytes(3, "big")
    f[4], f[5], f[6] = raw_lat >> 15, (raw_lat >> 7) & 0xFF, ((raw_lat & 0x7F) << 1) | (raw_lon >> 23)
    f[7], f[8], f[9] = (raw_lon >> 15) & 0xFF, (raw_lon >> 7) & 0xFF, (raw_lon & 0x7F) << 1
    f[10], f[11] = raw_alt >> 4, ((raw_alt & 15) << 4) | nic
    f[12], f[13] = (ag << 6) | (raw_a >> 6), ((raw_a & 0x3F) << 2) | (raw_b >> 9)
    f[14], f[15], f[16] = (raw_b >> 1) & 0xFF, ((raw_b & 1) << 7) | (raw_v >> 4), (raw_v & 15) << 4
    if callsign is not None:
        idx = [UG.BASE40.index(c) for c in callsign.ljust(8)]
        words = [idx[0] * 40 + idx[1], idx[2] * 1600 + idx[3] * 40 + idx[4], idx[5] * 1600 + idx[6] * 40 + idx[7]]
        for w, v in enumerate(words):
            f[17 + 2 * w], f[18 + 2 * w] = v >> 8, v & 0xFF
        f[26] = 0x02 if csid else 0
    return bytes(f)


def sticky_payloads():
    """Two addresses; after a first full frame, each later frame of an address carries only some fields (or none), so the aircraft
    keeps the others from before: the wrapper's 'copy only what is valid'."""
    full = dict(raw_lat=2200000, raw_lon=11000000, nic=8, raw_alt=150, raw_a=101, raw_b=51, raw_v=0x10A)
    up = bytearray(432)
    up[:18] = sv_payload(A1, 0, raw_alt=300)  # an uplink whose bytes 1-3 name A1: the wrapper decodes it as an MDB too
    return [
        sv_payload(A1, 1, callsign="ABC123", **full),                      # everything, with the call sign
        sv_payload(A1, 0),                                                 # nothing valid: airborne, no position, altitude, velocity
        sv_payload(A2, 0, raw_lat=100, raw_lon=200, nic=5, raw_alt=90, raw_a=0x400 | 30, raw_b=7),
        sv_payload(A1, 0, raw_alt=222),                                    # altitude only
        sv_payload(A1, 2, ag=2, raw_a=21, raw_b=(2 << 9) | 0x55),           # on the ground: speed and heading; vertical rate kept
        sv_payload(A1, 1, callsign="XYZ", csid=False, raw_lat=5, nic=0),   # CSID clear: a squawk, not a call sign; position from lat alone
        sv_payload(A1, 3, callsign="", raw_lon=77),                        # call sign all spaces: not valid
        bytes([11 << 3]) + A1.to_bytes(3, "big") + bytes(range(1, 31)),    # type 11: header only
        sv_payload(A2, 0, raw_a=12, raw_v=0x205),                          # north/south only: no speed, no track; vertical rate
        sv_payload(A1, 0, ag=1, raw_a=0x400 | 9, raw_b=0x400 | 3),          # supersonic: speed and track x 4
        bytes(up),
        sv_payload(A2, 1, callsign="N2", nic=1),                           # position (0, 0) valid through nic; call sign for A2
        sv_payload(A1, 0, ag=3, raw_a=500, raw_b=500, raw_v=0x1FF),         # reserved air/ground state: no velocity at all
    ]


def test_sticky_stream_demodulates_and_keeps_fields_across_frames():
    payloads = sticky_payloads()
    iq = UG.stream_of(payloads)
    o = O.Oracle978()
    frames = []
    for k in range(0, iq.size, UG.CALL_BYTES):
        frames += o.handle_data(iq[k:k + UG.CALL_BYTES])
    assert [p for _, p, _, _ in frames] == payloads and frames[10][0] == "+"
    mdbs, rows = M.Tracker().run(frames)
    # the case is worth testing: some later frames leave fields out that the aircraft still shows, and a stateless tracker or one
    # that copies invalid fields would print something else
    kept = dict(zip(M.Tracker.FIELDS, rows[1]))
    assert mdbs[1]["valid"] == M.V_SV and rows[1] == rows[0]
    assert kept["callsign"].rstrip(b"\0") == b"ABC123" and kept["altitude"] != 0 and kept["speed"] != 0 and kept["vert_rate"] != 0
    assert all(r[1].rstrip(b"\0") == b"ABC123" for r, m in zip(rows, mdbs) if r[0] == A1)
    assert rows[4][7] == rows[0][7] and rows[4][5] == 20  # ground frame: speed replaced, vertical rate kept
    assert rows[12][1:] == rows[10][1:]  # reserved state: nothing changes


def test_tracking_entry_points_reject_bad_arguments(native_libs):
    L = A.lib()
    n = C.c_uint64()
    assert L.adsb_amd_uat_set_tracking(None, None, None, 0) == -2
    assert L.adsb_amd_uat_aircraft_count(None, C.byref(n)) == -2
    assert L.adsb_amd_uat_reset_aircraft(None) == -2
    assert L.adsb_amd_uat_mdb_decode(None, 1, 27, None) == -2
    assert L.adsb_amd_uat_mdb_decode(None, 0, 0, None) == -2
    assert L.adsb_amd_uat_mdb_decode_device(None, None, 1, 27, None) == -2
