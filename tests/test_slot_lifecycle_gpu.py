"""The life of a result slot through the C ABI: submit, the fetches (whole, split into _begin / _end, to device memory on a caller's stream), refused
fetches and resubmits, in the orders the library allows and in the ones it must refuse.  Every scan's records are compared with a reference: the
oracle at 8 and 40 buffers (oracle/expected1090.c, held to helpers.expected_records by test_gpu_parity; oracle/oracle2400.c, the 2.4 MS/s mode's
specification), and at 1 024 buffers the same input through serial submit / fetch on a fresh Scanner, the path the parity tests hold to the oracle.

A scan's ordering pass does more than order its records: it zeroes the slot's work counters and the block-sum array the slot's NEXT scan adds into
(gather1090.hip.h).  A path that ends a scan without that pass lets the next scan skip chunks or misplace its records -- and read past its arrays --
without an error, so every test that resubmits a slot after such a path first asks adsb_amd_debug_slot_dirty whether the slot is clean."""
import pytest

import libadsb_amd as A
from libadsb_amd import synth
from oracle import oracle_py as O

import helpers as H

pytestmark = pytest.mark.gpu
BB = A.REF_BUFFER_BYTES
MODES = [pytest.param(A.MODE_2000, id="2000"), pytest.param(A.MODE_2400, id="2400")]
OUT_ALL = A.OUT_RECORDS | A.OUT_DECODED | A.OUT_PACKED
# three inputs a slot's scans cycle through: different densities, so that their record counts differ and a mix-up cannot pass on the count alone
CFGS = [dict(), dict(mean_spacing=300, noise_amp=8), dict(mean_spacing=900)]


class Case:
    """The three inputs of one mode and size on the device, with their reference records (and the packed form of them)."""

    def __init__(self, mode, nbuf):
        import torch
        rate = 24 if mode == A.MODE_2400 else 20
        self.mode, self.nbuf = mode, nbuf
        host = [synth.fill_range(31000 + 5000 * k, nbuf, cfg=synth.default_cfg(**cfg), nthreads=16, rate_x10=rate)[0] for k, cfg in enumerate(CFGS)]
        self.dev = [torch.from_numpy(x).cuda() for x in host]
        torch.cuda.synchronize()
        if nbuf <= 64:
            exp = O.expected_records2400 if mode == A.MODE_2400 else O.expected_records
            self.rec = [exp(x, BB, dtype=A.RECORD_DTYPE) for x in host]
            self.packed = [A.pack_records(r, A.decode_records_host(r)) for r in self.rec]
        else:
            sc = A.Scanner(mode=mode)
            sc.set_outputs(OUT_ALL)
            self.rec, self.packed = [], []
            for d in self.dev:
                sc.submit(d.data_ptr(), d.numel(), BB, 0, 0)
                self.rec.append(sc.fetch(0))
                sc.submit(d.data_ptr(), d.numel(), BB, 0, 0)
                self.packed.append(sc.fetch_packed(0))
            sc.close()
        assert len({len(r) for r in self.rec}) == 3 and min(len(r) for r in self.rec) > 0

    def args(self, k):
        return self.dev[k].data_ptr(), self.dev[k].numel(), BB


_cases = {}


def case(mode, nbuf):
    key = (mode, nbuf)
    if key not in _cases:
        for k in [k for k in _cases if k[1] > 64]:  # (one large case at a time: 768 MiB of inputs each)
            del _cases[k]
        _cases[key] = Case(mode, nbuf)
    return _cases[key]


@pytest.fixture(scope="module", autouse=True)
def _drop_cases():
    yield
    _cases.clear()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _same(got, want, what):
    """Byte for byte, records or the packed form."""
    assert got.dtype == want.dtype
    if len(got) == len(want) and got.tobytes() == want.tobytes():
        return
    bad = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), None)
    raise AssertionError("%s: %d records, the reference has %d%s" % (what, len(got), len(want), "" if bad is None else
                                                                      "; first difference at %d:\n got  %r\n want %r" % (bad, got[bad], want[bad])))


def _device_dst(nrec):
    import torch
    return torch.zeros(max(1, nrec) * 32, dtype=torch.uint8, device="cuda")


# The fetches the library refuses because the slot's scan did not produce the array asked for: (name, outputs of the refused scan, the call).
# Each consumes the scan.  (The device fetches check after waiting for the scan, the others before it.)
REFUSALS = [
    ("fetch", A.OUT_PACKED, lambda sc, slot, dst: sc.fetch(slot)),
    ("fetch_decoded", A.OUT_RECORDS | A.OUT_PACKED, lambda sc, slot, dst: sc.fetch_decoded(slot)),
    ("fetch_packed", A.OUT_RECORDS | A.OUT_DECODED, lambda sc, slot, dst: sc.fetch_packed(slot)),
    ("fetch_packed_begin", A.OUT_RECORDS | A.OUT_DECODED, lambda sc, slot, dst: sc.fetch_packed_begin(slot)),
    ("fetch_device", A.OUT_PACKED, lambda sc, slot, dst: sc.fetch_device(slot, dst.data_ptr(), dst.numel() // 32, _stream())),
    ("fetch_device_packed", A.OUT_RECORDS, lambda sc, slot, dst: sc.fetch_device(slot, dst.data_ptr(), dst.numel() // 32, _stream(), packed=True)),
]
REFUSAL_IDS = [r[0] for r in REFUSALS]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("refusal", REFUSALS, ids=REFUSAL_IDS)
def test_a_refused_fetch_leaves_the_slot_clean(native_libs, mode, refusal):
    """The slot invariant the tests below rest on: after a fetch the library refuses, of a slot that has had a fetched scan before, the slot's
    work counters and the sum array its next scan adds into are zero -- the refused scan's ordering pass has run -- and the scan is consumed.
    The hook itself refuses while the slot has a scan in flight."""
    name, outputs, refuse = refusal
    c = case(mode, 40)
    sc = A.Scanner(mode=mode)
    dst = _device_dst(max(len(r) for r in c.rec))
    slot, st = 1, _stream()
    assert sc.debug_slot_dirty(slot) == 0
    sc.submit(*c.args(0), st, slot)
    with pytest.raises(A.AdsbAmdError, match="in flight"):
        sc.debug_slot_dirty(slot)
    H.assert_records_equal(sc.fetch(slot), c.rec[0])
    assert sc.debug_slot_dirty(slot) == 0
    sc.set_outputs(outputs)
    sc.submit(*c.args(1), st, slot)
    with pytest.raises(A.AdsbAmdError, match="did not produce"):
        refuse(sc, slot, dst)
    assert sc.debug_slot_dirty(slot) == 0, "%s refused: the scan's ordering pass did not run, the slot's next scan would start on stale counters and sums" % name
    with pytest.raises(A.AdsbAmdError, match="fetch without submit"):
        sc.fetch(slot)  # the refusal consumed the scan
    sc.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nbuf", [8, 40, 1024])
def test_scans_after_a_refused_fetch_equal_their_references(native_libs, mode, nbuf):
    """For every refusal: scan X1 fetched, scan X2 refused, then X3 and X4 fetched -- each equal to its reference (X4: both of the slot's sum
    arrays have recovered).  Once as it stands, once with a submit on another slot of the same stream right behind the refusal (the refused
    scan's ordering pass must run, in that kernel or on its own, and not be lost).  One scanner throughout: the slot's history piles up."""
    c = case(mode, nbuf)
    sc = A.Scanner(mode=mode)
    dst = _device_dst(max(len(r) for r in c.rec))
    a, b, st = 0, 1, _stream()
    for other in (False, True):
        for name, outputs, refuse in REFUSALS:
            where = "%s refused%s, %d buffers" % (name, " then a submit on another slot" if other else "", nbuf)
            sc.set_outputs(OUT_ALL)
            sc.submit(*c.args(0), st, a)
            H.assert_records_equal(sc.fetch(a), c.rec[0])
            sc.set_outputs(outputs)
            sc.submit(*c.args(1), st, a)
            with pytest.raises(A.AdsbAmdError, match="did not produce"):
                refuse(sc, a, dst)
            sc.set_outputs(OUT_ALL)
            if other:
                sc.submit(*c.args(1), st, b)
            assert sc.debug_slot_dirty(a) == 0, where + ": the slot is not clean"
            sc.submit(*c.args(2), st, a)
            _same(sc.fetch_packed(a), c.packed[2], where + ": the next scan")
            sc.submit(*c.args(0), st, a)
            _same(sc.fetch(a), c.rec[0], where + ": the scan after it")
            if other:
                _same(sc.fetch(b), c.rec[1], where + ": the other slot's scan")
            assert sc.debug_slot_dirty(a) == 0 and sc.debug_slot_dirty(b) == 0
    sc.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nbuf", [40, 1024])
def test_split_fetch_misuse(native_libs, mode, nbuf):
    """Between fetch_packed_begin(A) and its _end:
    * a submit of A, then a submit of another slot B on the same stream: B's kernel must not take on the ordering pass of A's new scan (it would
      rewrite A's packed records under the copy) -- _end returns A's FIRST input, the later fetches the second input and B's;
    * a submit of A, then every fetch of A: each is refused as begun and not ended, without consuming the scan -- _end returns the first input,
      a fetch after it the second."""
    c = case(mode, nbuf)
    sc = A.Scanner(mode=mode)
    sc.set_outputs(OUT_ALL)
    dst = _device_dst(max(len(r) for r in c.rec))
    a, b, st = 0, 1, _stream()
    for rnd in range(2):  # (twice: the second round starts from the state the first left)
        sc.submit(*c.args(0), st, a)
        n = sc.fetch_packed_begin(a)
        sc.submit(*c.args(1), st, a)
        sc.submit(*c.args(2), st, b)
        first = sc.fetch_packed_end(a)
        assert n == len(first)
        _same(first, c.packed[0], "begin(A) submit(A) submit(B) end(A), %d buffers" % nbuf)
        _same(sc.fetch_packed(a), c.packed[1], "the scan of A submitted beside the copy")
        _same(sc.fetch(b), c.rec[2], "the scan of B")
    fetches = [("fetch", lambda: sc.fetch(a)), ("fetch_decoded", lambda: sc.fetch_decoded(a)), ("fetch_packed", lambda: sc.fetch_packed(a)),
               ("fetch_packed_begin", lambda: sc.fetch_packed_begin(a)),
               ("fetch_device", lambda: sc.fetch_device(a, dst.data_ptr(), dst.numel() // 32, st)),
               ("fetch_device_packed", lambda: sc.fetch_device(a, dst.data_ptr(), dst.numel() // 32, st, packed=True)),
               ("debug_slot_dirty", lambda: sc.debug_slot_dirty(a))]
    sc.submit(*c.args(0), st, a)
    n = sc.fetch_packed_begin(a)
    sc.submit(*c.args(2), st, a)
    for name, call in fetches:
        with pytest.raises(A.AdsbAmdError, match="begun and not ended"):
            call()
    first = sc.fetch_packed_end(a)
    assert n == len(first)
    _same(first, c.packed[0], "end(A) after the refused fetches, %d buffers" % nbuf)
    H.assert_records_equal(sc.fetch(a), c.rec[2])
    assert sc.debug_slot_dirty(a) == 0
    sc.close()


def _hold_cycles(target_ms=50.0):
    """Clock cycles for torch.cuda._sleep to hold a stream for about target_ms, from one timed call: at most target_ms whatever the counter's rate."""
    import torch
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(1000)  # (the first launch loads the kernel: not part of the timed call)
    torch.cuda.synchronize()
    t0.record()
    torch.cuda._sleep(1_000_000)
    t1.record()
    t1.synchronize()
    ms = t0.elapsed_time(t1)
    assert 0 < ms < 100, "torch.cuda._sleep(1e6) took %.3f ms" % ms
    return int(min(1_000_000 * target_ms / ms, 100_000_000))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nbuf", [40, 1024])
def test_device_fetch_on_a_held_stream_is_copied_before_the_slot_is_reordered(native_libs, mode, nbuf):
    """fetch_device(A, dst, S) returns with the copy queued on S, here behind a spin that holds S.  A's next scan, submitted right away, and
    then its ordering pass -- ridden in front of B's scan kernel, or launched on its own by fetch(A) -- rewrite A's dense arrays: the library must
    order the copy first.  dst holds A's first input.  (Whether the hold still runs when the calls return depends on the runtime: some calls have
    been seen to wait for the whole device.  The records are checked in every round either way.)"""
    import torch
    c = case(mode, nbuf)
    sc = A.Scanner(mode=mode)
    sc.set_outputs(OUT_ALL)
    side = torch.cuda.Stream()
    cap = max(len(r) for r in c.rec)
    a, b, st = 0, 1, _stream()
    # Before any stream is held: both slots' arrays made and grown to what the three inputs need (a slot's first scan allocates them, a scan whose
    # chunk overflowed its region reallocates them, and freeing device memory waits for the whole device), and a device fetch of each form.
    for _ in range(2):
        for slot in (a, b):
            for k in range(3):
                sc.submit(*c.args(k), st, slot)
                H.assert_records_equal(sc.fetch(slot), c.rec[k])
    for slot, packed in ((a, False), (b, True)):
        dst = _device_dst(cap)
        sc.submit(*c.args(0), st, slot)
        n = sc.fetch_device(slot, dst.data_ptr(), cap, side.cuda_stream, packed=packed)
        side.synchronize()
        want = c.packed[0] if packed else c.rec[0]
        _same(dst[:n * 32].cpu().numpy().view(want.dtype), want, "fetch_device on an idle stream")
    cycles = _hold_cycles()
    for packed, then in ((False, "submit(B)"), (True, "fetch(A)"), (True, "submit(B)"), (False, "fetch(A)")):
        dst = _device_dst(cap)
        sc.submit(*c.args(0), st, a)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            torch.cuda._sleep(cycles)
        n = sc.fetch_device(a, dst.data_ptr(), cap, side.cuda_stream, packed=packed)
        sc.submit(*c.args(1), st, a)
        if then == "submit(B)":
            sc.submit(*c.args(2), st, b)
            torch.cuda.synchronize()
            _same(sc.fetch(b), c.rec[2], "B")
            second = sc.fetch(a)
        else:
            second = sc.fetch(a)
            torch.cuda.synchronize()
        want = c.packed[0] if packed else c.rec[0]
        assert n == len(want)
        got = dst[:n * 32].cpu().numpy().view(want.dtype)
        _same(got, want, "fetch_device(A, S held) then submit(A), %s (%s, %d buffers): the device copy" % (then, "packed" if packed else "records", nbuf))
        H.assert_records_equal(second, c.rec[1])
        assert sc.debug_slot_dirty(a) == 0
    sc.close()


@pytest.mark.parametrize("mode", MODES)
def test_three_slots_over_two_streams_with_resubmits_beside_the_hosting_kernel(native_libs, mode):
    """The loop adsb_amd.h recommends, three slots alternating over two streams, 30 steps: two slots scan 1 024 buffers, the third 40.  The small
    scan's ordering pass rides in the large kernel behind it on its stream; its count reaches the host while that kernel still runs, and the slot is
    resubmitted at once, on the OTHER stream -- its scan adds into the sums and draws from the counters the pass has just zeroed, on other XCDs.
    Every step equals its own serial result.  (A regression guard: the zeroes are written through to memory, which is what makes this sound.)"""
    big, small = case(mode, 1024), case(mode, 40)
    import torch
    side = torch.cuda.Stream()
    sc = A.Scanner(mode=mode)
    sc.set_outputs(A.OUT_PACKED)
    sts = [_stream(), side.cuda_stream]
    inputs = [(big, 0), (big, 1), (small, 1)]
    steps = 30
    for k in range(3):
        cs, j = inputs[k]
        sc.submit(*cs.args(j), sts[k % 2], k)
    for i in range(steps):
        n = sc.fetch_packed_begin(i % 3)
        if i + 3 < steps:
            cs, j = inputs[(i + 3) % 3]
            sc.submit(*cs.args(j), sts[(i + 3) % 2], i % 3)
        rec = sc.fetch_packed_end(i % 3)
        assert len(rec) == n
        cs, j = inputs[i % 3]
        _same(rec, cs.packed[j], "step %d (%d buffers)" % (i, cs.nbuf))
    torch.cuda.synchronize()
    for k in range(3):
        assert sc.debug_slot_dirty(k) == 0
    sc.close()
