"""Test-side restatement of the UAT 978 MDB decoder and of the aircraft tracker built on it (libadsb_amd/csrc/mdb978.h and the
tracker in uat978_host.cpp), written from the published rules, not from that code.

decode_many(frames) follows dump978's legacy uat_decode_adsb_mdb as far as uat2json-wrapper.cpp:14-122 consumes it (header,
state vector, mode-status call sign); Tracker applies the wrapper's sticky copy per frame.  oracle/ cannot change, so this module is
the reference the product's decoder is held against.
"""
import math

import numpy as np

from oracle import oracle_py as O

BASE40 = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ  .."
V_SV, V_POSITION, V_ALTITUDE, V_SPEED, V_TRACK, V_VERTRATE, V_CALLSIGN = 1, 2, 4, 8, 16, 32, 64
MDB_BYTES = 27
MDB_DTYPE = np.dtype([("address", "<u4"), ("mdb_type", "u1"), ("valid", "u1"), ("track", "<u2"), ("lat1e7", "<i4"), ("lon1e7", "<i4"),
                      ("altitude", "<i4"), ("speed", "<u2"), ("vert_rate", "<i2"), ("callsign", "S8")])


def track_of(ns, ew):
    """(uint16_t)(360 + 90 - atan2(ns, ew) * 180 / M_PI) % 360 -- the value is in [270, 630), so the cast truncates a positive number."""
    return int(360 + 90 - math.atan2(ns, ew) * 180 / math.pi) % 360


def _tracks(ns, ew):
    """track_of over arrays.  numpy's arctan2 may differ from the C library's by an ulp, which cannot move the truncation where the
    angle is not a whole number of degrees (tests/test_uat978_track_cpu.py checks the margin); the directions where it is one
    (ns == 0, ew == 0, |ns| == |ew|) take math.atan2, the C library's, through the formula as written."""
    ns = np.asarray(ns, dtype=np.int64)
    ew = np.asarray(ew, dtype=np.int64)
    t = (360 + 90 - np.arctan2(ns.astype(np.float64), ew.astype(np.float64)) * 180 / math.pi).astype(np.int64) % 360
    special = (ns == 0) | (ew == 0) | (np.abs(ns) == np.abs(ew))
    for k in np.flatnonzero(special):
        t[k] = track_of(int(ns[k]), int(ew[k]))
    return t


def pad(frames):
    """(count, n) uint8 -> (count, 27): bytes past a frame's end read as 0 (a short frame has 18)."""
    f = np.asarray(frames, dtype=np.uint8)
    if f.ndim == 1:
        f = f[None, :]
    out = np.zeros((f.shape[0], MDB_BYTES), dtype=np.uint8)
    k = min(MDB_BYTES, f.shape[1])
    out[:, :k] = f[:, :k]
    return out


def decode_many(frames):
    """MDB_DTYPE[count] for a (count, n) uint8 array of corrected frame bytes."""
    f = pad(frames).astype(np.int64)
    n = f.shape[0]
    m = np.zeros(n, dtype=MDB_DTYPE)
    m["address"] = (f[:, 1] << 16) | (f[:, 2] << 8) | f[:, 3]
    t = f[:, 0] >> 3
    m["mdb_type"] = t
    valid = np.zeros(n, dtype=np.int64)
    sv = t <= 10  # types 0-10 carry a state vector; 11-31 only the header
    valid |= np.where(sv, V_SV, 0)

    raw_lat = (f[:, 4] << 15) | (f[:, 5] << 7) | (f[:, 6] >> 1)
    raw_lon = ((f[:, 6] & 1) << 23) | (f[:, 7] << 15) | (f[:, 8] << 7) | (f[:, 9] >> 1)
    nic = f[:, 11] & 15
    pos = sv & ((nic != 0) | (raw_lat != 0) | (raw_lon != 0))
    lat = raw_lat.astype(np.float64) * 360.0 / 16777216.0
    lat = np.where(lat > 90, lat - 180, lat)
    lon = raw_lon.astype(np.float64) * 360.0 / 16777216.0
    lon = np.where(lon > 180, lon - 360, lon)
    m["lat1e7"] = np.where(pos, np.trunc(lat * 10000000), 0).astype(np.int32)
    m["lon1e7"] = np.where(pos, np.trunc(lon * 10000000), 0).astype(np.int32)
    valid |= np.where(pos, V_POSITION, 0)

    raw_alt = (f[:, 10] << 4) | (f[:, 11] >> 4)
    alt = sv & (raw_alt != 0)
    m["altitude"] = np.where(alt, (raw_alt - 1) * 25 - 1000, 0)
    valid |= np.where(alt, V_ALTITUDE, 0)

    ag = f[:, 12] >> 6
    raw_a = ((f[:, 12] & 0x1F) << 6) | (f[:, 13] >> 2)
    raw_b = ((f[:, 13] & 3) << 9) | (f[:, 14] << 1) | (f[:, 15] >> 7)
    air = sv & (ag <= 1)
    scale = np.where(ag == 1, 4, 1)
    ns = ((raw_a & 0x3FF) - 1) * scale
    ns = np.where(raw_a & 0x400, -ns, ns)
    ew = ((raw_b & 0x3FF) - 1) * scale
    ew = np.where(raw_b & 0x400, -ew, ew)
    both = air & ((raw_a & 0x3FF) != 0) & ((raw_b & 0x3FF) != 0)
    speed = np.where(both, np.sqrt((ns * ns + ew * ew).astype(np.float64)).astype(np.int64), 0)
    air_track = both & ((ns != 0) | (ew != 0))
    track = np.zeros(n, dtype=np.int64)
    if air_track.any():
        track[air_track] = _tracks(ns[air_track], ew[air_track])
    raw_v = ((f[:, 15] & 0x7F) << 4) | (f[:, 16] >> 4)
    vr_ok = air & ((raw_v & 0x1FF) != 0)
    vr = ((raw_v & 0x1FF) - 1) * 64
    vr = np.where(raw_v & 0x200, -vr, vr)

    ground = sv & (ag == 2)
    g_speed = ground & ((raw_a & 0x3FF) != 0)
    g_track = ground & (((raw_b >> 9) & 3) != 0)
    speed = np.where(g_speed, (raw_a & 0x3FF) - 1, speed)
    track = np.where(g_track, (raw_b & 0x1FF) * 360 // 512, track)
    m["speed"] = speed
    m["track"] = track
    m["vert_rate"] = np.where(vr_ok, vr, 0)
    valid |= np.where(both | g_speed, V_SPEED, 0) | np.where(air_track | g_track, V_TRACK, 0) | np.where(vr_ok, V_VERTRATE, 0)

    ms = (t == 1) | (t == 3)
    for k in np.flatnonzero(ms):
        cs = callsign_of(f[k])
        if cs is not None:
            m["callsign"][k] = cs
            valid[k] |= V_CALLSIGN
    m["valid"] = valid
    return m


def callsign_of(f):
    """The mode-status call sign of a frame as the wrapper takes it (callsign_type == CS_CALLSIGN), or None."""
    words = [(int(f[17 + 2 * w]) << 8) | int(f[18 + 2 * w]) for w in range(3)]
    chars = [BASE40[(words[0] // 40) % 40], BASE40[words[0] % 40]]
    for v in words[1:]:
        chars += [BASE40[(v // 1600) % 40], BASE40[(v // 40) % 40], BASE40[v % 40]]
    while chars and chars[-1] == " ":
        chars.pop()  # trailing spaces become NUL
    cs = "".join(chars).ljust(8, "\0")
    if cs[0] == "\0" or not (int(f[26]) & 0x02):
        return None
    return cs.encode("latin-1")


def decode(frame):
    return decode_many(np.frombuffer(bytes(frame), dtype=np.uint8)[None, :])[0]


class Tracker:
    """uat2json-wrapper.cpp:18-121: FindOrCreate by address, copy what the update marks valid, squawk stays 0."""

    FIELDS = ("addr", "callsign", "lat1e7", "lon1e7", "altitude", "speed", "track", "vert_rate", "squawk")

    def __init__(self):
        self.aircraft = {}

    def apply(self, m):
        addr = int(m["address"])
        a = self.aircraft.setdefault(addr, dict(addr=addr, callsign=b"\0" * 8, lat1e7=0, lon1e7=0, altitude=0, speed=0, track=0,
                                                vert_rate=0, squawk=0))
        v = int(m["valid"])
        if v & V_POSITION:
            a["lat1e7"], a["lon1e7"] = int(m["lat1e7"]), int(m["lon1e7"])
        if v & V_SPEED:
            a["speed"] = int(m["speed"])
        if v & V_ALTITUDE:
            a["altitude"] = int(m["altitude"])
        if v & V_TRACK:
            a["track"] = int(m["track"])
        if v & V_VERTRATE:
            a["vert_rate"] = int(m["vert_rate"])
        if v & V_CALLSIGN:
            a["callsign"] = bytes(m["callsign"]).ljust(8, b"\0")
        return tuple(a[k] for k in self.FIELDS)

    def run(self, frames):
        """frames: [(updown, payload bytes, rs_errors, sample_index)] as the oracle reports them -> (mdbs, aircraft rows)."""
        if not frames:
            return np.zeros(0, MDB_DTYPE), []
        arr = np.zeros((len(frames), MDB_BYTES), dtype=np.uint8)
        for k, (_, p, _, _) in enumerate(frames):
            q = bytes(p[:MDB_BYTES])
            arr[k, :len(q)] = np.frombuffer(q, dtype=np.uint8)
        mdbs = decode_many(arr)
        return mdbs, [self.apply(m) for m in mdbs]


def format_row(row):
    """A Tracker row (or an AIRCRAFT_DTYPE row) as the reference's test listener prints it."""
    if isinstance(row, tuple):
        addr, cs, lat, lon, alt, speed, _, _, squawk = row
    else:
        addr, cs, lat, lon, alt, speed, squawk = (int(row["addr"]), bytes(row["callsign"]), int(row["lat1e7"]), int(row["lon1e7"]),
                                                  int(row["altitude"]), int(row["speed"]), int(row["squawk"]))
    return O.format_aircraft(addr, cs, lat, lon, alt, speed, squawk)
