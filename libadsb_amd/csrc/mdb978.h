// mdb978.h -- dump978's uat_decode_adsb_mdb as far as uat2json-wrapper.cpp:14-122 consumes it: address, type, state vector
// (position, altitude, speed, track, vertical rate) and the mode-status call sign, as a pure function of the frame's first 27
// bytes.  The rules restate the published legacy uat_decode.c (un-vendored in the reference tree): parity beyond
// the reference's two 978 golden texts is unpinned.
//
// One source, two builds: uat_mdb_kernel (uat978.hip) runs it per reported frame on the device, the host runs it for frames that
// no kernel decoded (the host's own scan loop) and for the CPU tests.  Both must give the same bytes:
//   * integer fields are bit fiddling;
//   * lat/lon: raw * 360.0 / 2^24 is exact in double, the wrap subtracts exactly, and (int32_t)(deg * 1e7) is one correctly
//     rounded double multiply and a truncation -- the same on both sides (the build passes -ffp-contract=off);
//   * speed = (int)sqrt(ns^2 + ew^2) with the value below 2^25: the integer square root, computed with an integer fix-up;
//   * track = (uint16_t)(360 + 90 - atan2(ns, ew) * 180 / M_PI) % 360.  For |ns|, |ew| <= 1022 (x 4 when supersonic, which
//     scales both and leaves the angle alone) the angle is a whole number of degrees only on the eight directions ns = 0, ew = 0,
//     |ns| = |ew|; there both builds return the value the host's libm gives (90, 270, 0, 180, 45, 315, 135, 225) without calling
//     atan2.  Everywhere else the angle is at least 1.3e-6 degrees from a whole number (decode1090.h: exhaustive over a larger
//     lattice; tests/test_uat978_track_cpu.py re-checks it for this one), eight orders of magnitude above the error of a
//     double-precision atan2 on either side, so the truncation cannot differ.  Both builds use double atan2.
#pragma once

#include <math.h>
#include <stdint.h>

#include "adsb_amd.h"

#if defined(__HIPCC__)
#define ADSB_AMD_HD __host__ __device__
#else
#define ADSB_AMD_HD
#endif

namespace adsb_amd
{
using uat_mdb_t = adsb_amd_uat_mdb_t;
static_assert(sizeof(uat_mdb_t) == 32, "uat_mdb_t: one 32-byte record per frame");

constexpr int kUatMdbBytes = 27; // the decoder reads frame bytes 0..26 (mode status ends at byte 26)

ADSB_AMD_HD inline int uat_isqrt25(int n)
{ // floor(sqrt(n)), 0 <= n < 2^25
    int r = (int)sqrt((double)n);
    while (r * r > n) r--;
    while ((r + 1) * (r + 1) <= n) r++;
    return r;
}

// (uint16_t)(360 + 90 - atan2(ns, ew) * 180 / M_PI) % 360, see the header comment
ADSB_AMD_HD inline int uat_track_of(int ns, int ew)
{
    const int ans = ns < 0 ? -ns : ns, aew = ew < 0 ? -ew : ew;
    if (ns == 0) return ew > 0 ? 90 : 270;
    if (ew == 0) return ns > 0 ? 0 : 180;
    if (ans == aew) return ns > 0 ? (ew > 0 ? 45 : 315) : (ew > 0 ? 135 : 225);
    return (int)(uint16_t)(360 + 90 - atan2((double)ns, (double)ew) * 180 / 3.14159265358979323846) % 360;
}

ADSB_AMD_HD inline char uat_base40(unsigned v)
{ // "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ  .."
    return v < 10 ? (char)('0' + v) : v < 36 ? (char)('A' + (v - 10)) : v < 38 ? ' ' : '.';
}

// f: at least kUatMdbBytes bytes (a short frame's are zero past its 18)
ADSB_AMD_HD inline uat_mdb_t decode_mdb(const uint8_t* f)
{
    uat_mdb_t m;
    m.address  = ((uint32_t)f[1] << 16) | ((uint32_t)f[2] << 8) | f[3];
    m.mdb_type = (uint8_t)(f[0] >> 3);
    m.valid = 0, m.track = 0, m.lat1e7 = 0, m.lon1e7 = 0, m.altitude = 0, m.speed = 0, m.vert_rate = 0;
    for (int i = 0; i < 8; i++) m.callsign[i] = 0;
    const int t = m.mdb_type;
    if (t > 10) return m; // header only
    m.valid = ADSB_AMD_UAT_SV;
    { // position
        const uint32_t raw_lat = ((uint32_t)f[4] << 15) | ((uint32_t)f[5] << 7) | (f[6] >> 1);
        const uint32_t raw_lon = ((uint32_t)(f[6] & 1) << 23) | ((uint32_t)f[7] << 15) | ((uint32_t)f[8] << 7) | (f[9] >> 1);
        const int      nic     = f[11] & 15;
        if (nic || raw_lat || raw_lon)
        {
            double lat = raw_lat * 360.0 / 16777216.0, lon = raw_lon * 360.0 / 16777216.0;
            if (lat > 90) lat -= 180;
            if (lon > 180) lon -= 360;
            m.lat1e7 = (int32_t)(lat * 10000000);
            m.lon1e7 = (int32_t)(lon * 10000000);
            m.valid |= ADSB_AMD_UAT_POSITION;
        }
    }
    { // altitude
        const int raw_alt = (f[10] << 4) | (f[11] >> 4);
        if (raw_alt)
        {
            m.altitude = (raw_alt - 1) * 25 - 1000;
            m.valid |= ADSB_AMD_UAT_ALTITUDE;
        }
    }
    const int ag = f[12] >> 6;
    const int raw_a = ((f[12] & 0x1f) << 6) | (f[13] >> 2);                    // north/south velocity, or ground speed
    const int raw_b = ((f[13] & 3) << 9) | (f[14] << 1) | (f[15] >> 7);        // east/west velocity, or ground track
    if (ag <= 1)
    { // airborne; 1 = supersonic
        const int  scale = ag ? 4 : 1;
        const bool ns_ok = (raw_a & 0x3ff) != 0, ew_ok = (raw_b & 0x3ff) != 0;
        int        ns = ((raw_a & 0x3ff) - 1) * scale, ew = ((raw_b & 0x3ff) - 1) * scale;
        if (raw_a & 0x400) ns = -ns;
        if (raw_b & 0x400) ew = -ew;
        if (ns_ok && ew_ok)
        {
            if (ns || ew)
            {
                m.track = (uint16_t)uat_track_of(ns, ew);
                m.valid |= ADSB_AMD_UAT_TRACK;
            }
            m.speed = (uint16_t)uat_isqrt25(ns * ns + ew * ew);
            m.valid |= ADSB_AMD_UAT_SPEED;
        }
        const int raw_v = ((f[15] & 0x7f) << 4) | (f[16] >> 4);
        if (raw_v & 0x1ff)
        {
            int v = ((raw_v & 0x1ff) - 1) * 64;
            m.vert_rate = (int16_t)((raw_v & 0x200) ? -v : v);
            m.valid |= ADSB_AMD_UAT_VERTRATE;
        }
    }
    else if (ag == 2)
    { // on the ground
        if (raw_a & 0x3ff)
        {
            m.speed = (uint16_t)((raw_a & 0x3ff) - 1);
            m.valid |= ADSB_AMD_UAT_SPEED;
        }
        if ((raw_b >> 9) & 3)
        {
            m.track = (uint16_t)((raw_b & 0x1ff) * 360 / 512);
            m.valid |= ADSB_AMD_UAT_TRACK;
        }
    }
    if (t == 1 || t == 3)
    { // mode status: emitter category and eight characters, three base-40 digits per big-endian word
        char cs[8];
        for (int w = 0; w < 3; w++)
        {
            const unsigned v = ((unsigned)f[17 + 2 * w] << 8) | f[18 + 2 * w];
            if (w == 0)
                cs[0] = uat_base40((v / 40) % 40), cs[1] = uat_base40(v % 40);
            else
                cs[3 * w - 1] = uat_base40((v / 1600) % 40), cs[3 * w] = uat_base40((v / 40) % 40), cs[3 * w + 1] = uat_base40(v % 40);
        }
        for (int i = 7; i >= 0 && cs[i] == ' '; i--) cs[i] = 0;
        if (cs[0] && (f[26] & 0x02))
        {
            for (int i = 0; i < 8; i++) m.callsign[i] = cs[i];
            m.valid |= ADSB_AMD_UAT_CALLSIGN;
        }
    }
    return m;
}

// a frame of `len` bytes into the decoder's window, zero past its end
ADSB_AMD_HD inline uat_mdb_t decode_mdb_bytes(const uint8_t* data, int len)
{
    uint8_t f[kUatMdbBytes];
    for (int i = 0; i < kUatMdbBytes; i++) f[i] = i < len ? data[i] : 0;
    return decode_mdb(f);
}

} // namespace adsb_amd
