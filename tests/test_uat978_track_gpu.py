"""UAT 978 aircraft tracking on the GPU: the reference's two golden texts through Handler978 and through the C++ factory of a host
without dump978, the kernel build of the MDB decoder against the host build, and the update / aircraft sequence against the
test-side restatement (tests/uat_mdb.py) applied to the oracle's frames."""
import subprocess

import numpy as np
import pytest

import libadsb_amd as A
from libadsb_amd import synth
from oracle import oracle_py as O

import uat_golden_text as UG
import uat_mdb as M
from test_uat978_cpu import stale_register_case
from test_uat978_track_cpu import assert_mdb_equal, exhaustive_sets, sticky_payloads

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["short", "long"])
def golden(request):
    iq, _, lines = UG.build(request.param)
    return iq, lines


def text_of(aircraft):
    return [M.format_row(r) for r in aircraft]


@pytest.mark.parametrize("mode", ["whole", "calls", "process_iq", "aircraft_only"])
def test_handler978_prints_the_golden_text(native_libs, golden, mode):
    iq, lines = golden
    h = A.Handler978(want_frames=(mode != "aircraft_only"))
    if mode == "whole":
        _, ac = h.handle_data(iq)
    elif mode == "process_iq":
        _, ac, _ = h.process_iq(iq)
    else:
        parts = [h.handle_data(iq[k:k + UG.CALL_BYTES]) for k in range(0, iq.size, UG.CALL_BYTES)]
        ac = np.concatenate([a for _, a in parts])
    assert text_of(ac) == lines
    assert h.aircraft_count() == len({ln.split("[")[0] for ln in lines})
    h.close()


def test_cxx_factory_without_dump_raw_message_prints_the_golden_text(native_libs, golden, tmp_path):
    """ADSB::test::TryCreateUAT978Handler in a binary that defines no dump_raw_message: the handler tracks aircraft itself and the
    traffic manager's listener sees one OnChanged per frame, formatted as the reference's test formats it."""
    from libadsb_amd import build
    build.build_cxx_test()
    iq, lines = golden
    path = tmp_path / "978.iq"
    iq.tofile(path)
    out = subprocess.run([build.CXX_TEST_978_TRACK, str(path), str(UG.CALL_BYTES)], capture_output=True, timeout=300)
    assert out.returncode == 0, out.stderr.decode()
    assert out.stdout.decode("latin-1").split("\n")[:-1] == lines


def test_device_decoder_equals_the_host_decoder_on_exhaustive_sets(native_libs):
    u = A.Uat978()
    for label, f in exhaustive_sets():
        assert_mdb_equal(A.uat_mdb_decode(f, u), A.uat_mdb_decode(f), label)
    u.close()


def expected(frames):
    """The restatement on the oracle's frames: (updates as tuples, aircraft rows)."""
    mdbs, rows = M.Tracker().run(frames)
    ups = [(ud, rs, idx) + tuple(m[k].item() if k != "callsign" else bytes(m[k]) for k in M.MDB_DTYPE.names)
           for (ud, _, rs, idx), m in zip(frames, mdbs)]
    return ups, rows


def got_of(updates, aircraft):
    ups = [(u["updown"].decode(), int(u["rs_errors"]), int(u["sample_index"])) +
           tuple(u["mdb"][k].item() if k != "callsign" else bytes(u["mdb"][k]) for k in M.MDB_DTYPE.names) for u in updates]
    rows = [tuple(r[k].item() if k != "callsign" else bytes(r[k]).ljust(8, b"\0") for k in M.Tracker.FIELDS) for r in aircraft]
    return ups, rows


def assert_tracking(got, want):
    gu, gr = got
    wu, wr = want
    assert len(gu) == len(wu)
    for k, (a, b) in enumerate(zip(gu, wu)):
        assert a == b, (k, a, b)
    assert gr == [tuple(x if not isinstance(x, bytes) else x.ljust(8, b"\0") for x in r) for r in wr]


@pytest.mark.parametrize("stream,cfg_over", [
    (0, {}),
    (1, {"noise_amp": 6, "pct_corrupt": 60, "max_bad_bytes": 8}),
    (2, {"pct_uplink": 50, "mean_gap_bits": 300}),
    (3, {"amp_lo": 6, "amp_hi": 14, "noise_amp": 4}),
    (4, {"mean_gap_bits": 40, "pct_uplink": 0}),
])
def test_synth_streams_track_as_the_restatement_of_the_oracle_frames(native_libs, stream, cfg_over):
    """Uplinks decode as MDBs too (the wrapper ignores updown); frames and updates interleave in stream order."""
    iq = synth.fill978(stream, 6 * 262144, synth.default_cfg978(**cfg_over))
    h, o = A.Handler978(), O.Oracle978()
    frames, got_u, got_a = [], [], []
    for k in range(6):
        part = iq[k * 262144:(k + 1) * 262144]
        fr = A.Uat978.handle_data(h, part)  # the frame callbacks of a tracking handle ...
        u, a = h.take()                     # ... and its updates, in the same calls
        want = o.handle_data(part)
        assert fr == want
        frames += want
        got_u.append(u), got_a.append(a)
    assert len(frames) > 20
    assert_tracking(got_of(np.concatenate(got_u), np.concatenate(got_a)), expected(frames))
    h.close()


def test_frames_behind_frames_and_the_host_loop_track_as_the_restatement(native_libs):
    """The stale-register extras (decoded by uat_mdb_kernel from their side array), the same with no room for them (the host's own
    loop, positions it asks for decoded on the host) and a long stream on the host loop throughout."""
    phi, _, _ = stale_register_case()
    want = expected(O.process_buffer978(phi)[0])
    assert len(want[0]) == 2
    for setup in ("device", "no_extra_room", "host_loop"):
        for frames_wanted in (True, False):
            h = A.Handler978(want_frames=frames_wanted)
            if setup == "no_extra_room":
                h.set_extra_capacity(0)
            if setup == "host_loop":
                h.set_host_loop(True)
            h.process_phases(phi)
            assert_tracking(got_of(*h.take()), want)
            h.close()
    iq = synth.fill978(21, 32 << 20, synth.default_cfg978(pct_corrupt=30, max_bad_bytes=7, pct_uplink=20))
    frames, _ = O.process_buffer978(O.phase_lut978()[iq.view(np.uint16)])
    for frames_wanted in (True, False):
        h = A.Handler978(want_frames=frames_wanted)
        h.set_host_loop(True)
        assert_tracking(got_of(*h.process_iq(iq)[:2]), expected(frames))
        h.close()


def test_tracking_leaves_the_frame_callbacks_as_they_are(native_libs):
    iq = synth.fill978(9, 6 * 262144, synth.default_cfg978(pct_uplink=30))
    u, h = A.Uat978(), A.Handler978()
    for k in range(6):
        part = iq[k * 262144:(k + 1) * 262144]
        assert A.Uat978.handle_data(h, part) == u.handle_data(part)
    assert u.process_iq(iq) == A.Uat978.process_iq(h, iq)
    h.set_frames(False)
    assert A.Uat978.process_iq(h, iq)[0] == []  # aircraft only: no frame callbacks
    u.close(), h.close()


def test_tracking_calls_in_flight_equal_the_serial_calls(native_libs):
    import torch
    streams = [synth.fill978(40 + k, (4 + 2 * k) * 1024 * 1024, synth.default_cfg978(**over))
               for k, over in enumerate(({}, {"pct_uplink": 40}, {"mean_gap_bits": 40, "pct_corrupt": 60}, {}, {"noise_amp": 6}))]
    dev = [torch.from_numpy(x).cuda() for x in streams]
    torch.cuda.synchronize()
    for frames_wanted in (True, False):
        serial = A.Handler978(want_frames=frames_wanted)
        want = []
        for k, (d, x) in enumerate(zip(dev, streams)):
            fr = serial.process_device(d.data_ptr(), x.size // 2, offset=1000 * k)
            want.append((fr, got_of(*serial.take())))
        h = A.Handler978(want_frames=frames_wanted)
        ahead = h.max_in_flight() - 1
        for k in range(ahead):
            h.submit_device(dev[k].data_ptr(), streams[k].size // 2, 1000 * k)
        got = []
        for k in range(len(streams)):
            if k + ahead < len(streams):
                h.submit_device(dev[k + ahead].data_ptr(), streams[k + ahead].size // 2, 1000 * (k + ahead))
            fr = h.collect()
            got.append((fr, got_of(*h.take())))
        assert got == want
        assert h.aircraft_count() == serial.aircraft_count() > 0
        serial.close(), h.close()


def test_1gib_stream_aircraft_only_gives_the_aircraft_of_the_frames_mode(native_libs):
    import torch
    piece = 64 << 20
    dev = torch.empty(16 * piece, dtype=torch.uint8, device="cuda")
    for k in range(16):
        dev[k * piece:(k + 1) * piece].copy_(torch.from_numpy(synth.fill978(100 + k, piece, synth.default_cfg978())))
    torch.cuda.synchronize()
    out = []
    for frames_wanted in (True, False):
        h = A.Handler978(want_frames=frames_wanted)
        fr = h.process_device(dev.data_ptr(), dev.numel() // 2)
        up, ac = h.take()
        assert len(up) > 50000 and (len(fr[0]) == len(up) if frames_wanted else fr[0] == [])
        out.append((up.tobytes(), ac.tobytes(), h.aircraft_count()))
        h.reset_aircraft()
        assert h.aircraft_count() == 0
        h.close()
    assert out[0] == out[1]


def test_sticky_rule_on_every_path(native_libs, tmp_path):
    """Repeated addresses whose later frames leave fields out (tests/test_uat978_track_cpu.py: sticky_payloads): the aircraft keep
    what no later frame marks valid -- through HandleData whole and in live-sized calls, one process_buffer, aircraft only, the host
    loop, calls in flight (the same stream four times: the state carries across calls), and the C++ factory of a host without
    dump_raw_message (the traffic manager's own aircraft)."""
    import torch
    from libadsb_amd import build
    iq = UG.stream_of(sticky_payloads())
    n = iq.size // 2
    once, _ = O.process_buffer978(O.phase_lut978()[iq.view(np.uint16)])

    def oracle_calls(step):  # the sample indices of HandleData count the samples it consumed: the oracle, called the same way
        o = O.Oracle978()
        return [f for k in range(0, iq.size, step) for f in o.handle_data(iq[k:k + step])]

    by_step = {step: expected(oracle_calls(step)) for step in (iq.size, UG.CALL_BYTES)}
    for path in ("whole", "calls", "process_iq", "aircraft_only", "host_loop"):
        want = expected(once) if path in ("process_iq", "host_loop") else by_step[UG.CALL_BYTES if path == "calls" else iq.size]
        h = A.Handler978(want_frames=(path != "aircraft_only"))
        if path == "host_loop":
            h.set_host_loop(True)
        if path in ("whole", "aircraft_only"):
            got = h.handle_data(iq)
        elif path == "calls":
            parts = [h.handle_data(iq[k:k + UG.CALL_BYTES]) for k in range(0, iq.size, UG.CALL_BYTES)]
            got = (np.concatenate([u for u, _ in parts]), np.concatenate([a for _, a in parts]))
        else:
            got = h.process_iq(iq)[:2]
        assert_tracking(got_of(*got), want)
        h.close()

    four = [(ud, p, rs, idx + k * n) for k in range(4) for ud, p, rs, idx in once]
    want4 = expected(four)
    dev = torch.from_numpy(iq).cuda()
    torch.cuda.synchronize()
    for frames_wanted in (True, False):
        h = A.Handler978(want_frames=frames_wanted)
        ahead = h.max_in_flight() - 1
        for k in range(ahead):
            h.submit_device(dev.data_ptr(), n, k * n)
        parts = []
        for k in range(4):
            if k + ahead < 4:
                h.submit_device(dev.data_ptr(), n, (k + ahead) * n)
            h.collect()
            parts.append(h.take())
        assert_tracking(got_of(np.concatenate([u for u, _ in parts]), np.concatenate([a for _, a in parts])), want4)
        h.close()

    build.build_cxx_test()
    path = tmp_path / "sticky.iq"
    iq.tofile(path)
    out = subprocess.run([build.CXX_TEST_978_TRACK, str(path), str(UG.CALL_BYTES)], capture_output=True, timeout=120)
    assert out.returncode == 0, out.stderr.decode()
    assert out.stdout.decode("latin-1").split("\n")[:-1] == [M.format_row(r) for r in by_step[UG.CALL_BYTES][1]]
