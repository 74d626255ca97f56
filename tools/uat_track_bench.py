"""What aircraft tracking costs on the UAT 978 path: the bench's 1 GiB synth.fill978 stream (device resident, one process_buffer per
call, three calls in flight), for frames only (an untracked handle), frames + aircraft, and aircraft only.

    python tools/uat_track_bench.py [--steps N] [--modes frames,both,aircraft]

Per mode: ms per call (three in flight and back to back), the bytes copied device -> host per call -- COMPUTED from counts, not
measured: 16 B record + 40 B frame bytes per match, 432 B per reported uplink frame (the copy takes every decoded uplink slot, so this
part is a lower bound), 32 B decoded MDB per match when tracking; the marks and counts are left out --
and the host's walk over the frames taken (host_wall_ms.loop: with tracking this is the tracker, with a native no-op callback).
The uat_mdb_kernel time comes from a separate run under rocprofv3 --kernel-trace --stats (profiles/).  One JSON line per mode.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import libadsb_amd as A  # noqa: E402
from libadsb_amd import synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--modes", default="frames,both,aircraft")
args = ap.parse_args()

piece, npieces = 64 << 20, 16
cfg = synth.default_cfg978()
dev = torch.empty(npieces * piece, dtype=torch.uint8, device="cuda")
with ThreadPoolExecutor(npieces) as ex:
    for k, h in enumerate(ex.map(lambda k: synth.fill978(100 + k, piece, cfg), range(npieces))):
        dev[k * piece:(k + 1) * piece].copy_(torch.from_numpy(h))
torch.cuda.synchronize()
n = dev.numel() // 2
L = A.lib()

# what one call reports: matches, and frames by kind (one frames-mode call with the frames collected)
probe = A.Uat978(0)
before = probe.timing()["candidates"]
frames, _ = probe.process_device(dev.data_ptr(), n)
ncand = probe.timing()["candidates"] - before
nup = sum(1 for f in frames if f[0] == "+")
probe.close()


def run(mode):
    u = A.Uat978(0)
    counter = C.c_uint64(0)
    if mode != "frames":  # the library's counting callback has the tracking callback's shape (three pointers): a native no-op listener
        rc = L.adsb_amd_uat_set_tracking(u._h, C.cast(L.adsb_amd_count_callback, C.c_void_p), C.cast(C.pointer(counter), C.c_void_p),
                                         0 if mode == "aircraft" else 1)
        assert rc == 0
    for _ in range(5):
        u.process_device(dev.data_ptr(), n, collect=False)
    t0 = time.perf_counter()
    loop = 0.0
    for _ in range(args.steps):
        u.process_device(dev.data_ptr(), n, collect=False)
        loop += u.timing()["host_wall_ms"]["loop"]
    serial = (time.perf_counter() - t0) / args.steps * 1e3
    ahead = u.max_in_flight() - 1
    t0 = time.perf_counter()
    for _ in range(ahead):
        u.submit_device(dev.data_ptr(), n)
    for i in range(args.steps):
        if i + ahead < args.steps:
            u.submit_device(dev.data_ptr(), n)
        u.collect(collect=False)
    pipelined = (time.perf_counter() - t0) / args.steps * 1e3
    per_call = counter.value / (2 * args.steps + 5) if mode != "frames" else 0
    u.close()
    d2h = 16 * ncand + (40 * ncand + 432 * nup if mode != "aircraft" else 0) + (32 * ncand if mode != "frames" else 0)
    return {"mode": mode, "ms_per_call_three_in_flight": round(pipelined, 4), "ms_per_call_back_to_back": round(serial, 4),
            "bytes_d2h_per_call_computed": d2h, "host_loop_ms_per_call": round(loop / args.steps, 4), "updates_per_call": per_call,
            "matches_per_call": ncand, "frames_per_call": len(frames), "uplink_frames_per_call": nup, "gib_per_call": dev.numel() / 2**30}


for mode in args.modes.split(","):
    print(json.dumps(run(mode)), flush=True)
