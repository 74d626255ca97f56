"""The stand-alone slice of libadsb's surface (include/libadsb_iface.hpp) against the reference's own headers.

tests/cpp/iface_layout.cpp prints, one fact per line, what a caller compiled against either header set relies on: Source's enumerators,
every IAirCraft / IListener / IDataProvider member-function signature and virtual-table slot (the order of the virtual functions),
sizeof / alignof of every type, type and offsetof of AirCraftImpl's and TrafficManager's data members, TrafficManager::FindOrCreate /
SetListener / NotifyChanged and its base.  Built against the reference's ADSBListener.h and AircraftImpl.h (ADSBListener.h:27-72,
AircraftImpl.h:9-68) its output is the stored tests/golden/iface_reference_layout.txt; built against the stand-alone header it must print
the same text.  Where oracle/_ref/iface_layout has been built from a reference checkout (oracle/Makefile), its output is held to the stored
text as well.
"""
import difflib
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "iface_reference_layout.txt")
REF_BUILD = os.path.join(ROOT, "oracle", "_ref", "iface_layout")


def _diff(got, want, got_name):
    return "".join(difflib.unified_diff(want.splitlines(True), got.splitlines(True), "iface_reference_layout.txt", got_name))


def test_standalone_interface_equals_the_reference_headers(tmp_path):
    want = open(GOLDEN).read()
    exe = str(tmp_path / "iface_layout")
    cmd = ["g++", "-std=c++20", "-Wall", "-Wextra", "-Wno-invalid-offsetof", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "iface_layout.cpp"), "-o", exe]
    cc = subprocess.run(cmd, capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout == want, "libadsb_iface.hpp no longer matches the reference headers:\n" + _diff(run.stdout, want, "libadsb_iface.hpp")
    if os.path.exists(REF_BUILD):
        ref = subprocess.run([REF_BUILD], capture_output=True, text=True)
        assert ref.returncode == 0 and ref.stdout == want, "the stored layout differs from the reference's own:\n" + _diff(ref.stdout, want, "oracle/_ref/iface_layout")
