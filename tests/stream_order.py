"""Helpers that put the `stream` argument of the C ABI to the test (include/szg/abi.h: "enqueued on `stream`, returns
immediately", and the STREAM RULE about the device state a pipeline object rewrites in stream order).

Every other GPU test records on torch's current stream, which is the legacy null stream, or on a blocking stream with
nothing in front of it: a kernel, memset or copy that went to stream 0 instead of the caller's stream is ordered correctly
there by accident. Here a case runs on a stream that is KNOWN to be non-blocking (created through HIP, flag read back), in two
arrangements, each after a warm run of the same case on the same pipeline objects:

  behind  a blocker runs on the side stream S; then, on S, the inputs are written, the outputs prefilled with the sentinels
          of tests/padded_images.py and the pass recorded. Condition A: when the last record call has returned the blocker
          has not finished - so nothing of the case ran yet, and whatever part of the pass went to the null stream ran
          before its inputs existed.
  beside  the blocker runs on the NULL stream, inputs and pass on S, then S.synchronize(). Condition B: the blocker is still
          not complete when S.synchronize() has returned - so whatever part of the pass went to the null stream ran too
          late or made the call wait for the device.

A condition that does not hold FAILS the test as "inconclusive": it never passes or skips on that.

Inputs reach the device in stream order only: a case uploads what it needs into staging tensors BEFORE the blocker
(prepare()), and behind the blocker only enqueues device-to-device copies, pinned uploads of the pipelines' own staged
buffers and the record calls (enqueue()). No pageable copy, allocation or host sync stands behind the blocker, because each
of them may wait for the stream. The inputs of the three runs of a case differ, and every buffer of every run stays alive
until the case ends: an early or stale read then finds valid memory that holds other numbers, and shows as a wrong image,
never as a fault.

A case is an object with
  id                     its pytest id
  setup(gpu) -> state    the pipeline objects, created once per case
  prepare(gpu, state, variant) -> run    variant 0 = warm, 1 = behind, 2 = beside: inputs, expected result, staging tensors
  enqueue(gpu, state, run, S)            asynchronous work only, with S the current torch stream
  check(gpu, state, run, what)           after S.synchronize()
  teardown(gpu, state)
  conditions             False where a record call waits for the stream by design (stated by the case)

numpy and ctypes only until a GPU is asked for: the module imports on a machine without one."""
import contextlib
import ctypes as C
import gc
import math
import time
import traceback

import pytest

HIP_STREAM_NON_BLOCKING = 0x01
HIP_MEMCPY_DEVICE_TO_DEVICE = 3
MAX_STREAMS_PER_CASE = 3

# Blocker length: at least FLOOR_MS and MULTIPLIER x the wall time of the case's warm run (host time of the record calls
# plus the device time until S.synchronize() returns, which is never less than the host time alone: so this is also
# at least MULTIPLIER >= 4 x the host time), at most CEILING_MS. Condition B needs the device time in it: beside the
# blocker the pass shares the device with it and runs slower than alone. The margins observed on an MI355X are in
# profiles/stream_order_mutants.md.
MULTIPLIER = 8.0
FLOOR_MS = 25.0
CEILING_MS = 250.0
BLOCKER_ELEMENTS = 1 << 28  # float32: 1 GiB read and written by every op of the chain

_hip = None


def hip():
    """libamdhip64.so as it is already loaded in the process (torch's), with the few entry points used here."""
    global _hip
    if _hip is None:
        h = C.CDLL("libamdhip64.so")
        h.hipStreamCreateWithFlags.restype = C.c_int
        h.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
        h.hipStreamGetFlags.restype = C.c_int
        h.hipStreamGetFlags.argtypes = [C.c_void_p, C.POINTER(C.c_uint)]
        h.hipStreamDestroy.restype = C.c_int
        h.hipStreamDestroy.argtypes = [C.c_void_p]
        h.hipMemcpy2DAsync.restype = C.c_int
        h.hipMemcpy2DAsync.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p]
        _hip = h
    return _hip


def blocker_length_ms(warm_host_s, warm_total_s):
    """The rule above, in milliseconds."""
    assert warm_total_s >= warm_host_s >= 0.0
    return min(CEILING_MS, max(FLOOR_MS, MULTIPLIER * warm_total_s * 1e3))


@contextlib.contextmanager
def side_streams(torch, count=1):
    """`count` non-blocking streams as torch.cuda.ExternalStream, destroyed on exit. The flag is read back: on a blocking
    stream every test of this kind would pass for the wrong reason."""
    assert 1 <= count <= MAX_STREAMS_PER_CASE
    handles, streams = [], []
    try:
        for _ in range(count):
            h = C.c_void_p()
            rc = hip().hipStreamCreateWithFlags(C.byref(h), HIP_STREAM_NON_BLOCKING)
            assert rc == 0 and h.value, f"hipStreamCreateWithFlags failed: {rc}"
            handles.append(h)
            flags = C.c_uint(0)
            rc = hip().hipStreamGetFlags(h, C.byref(flags))
            assert rc == 0 and flags.value & HIP_STREAM_NON_BLOCKING, f"the side stream is not non-blocking (rc {rc}, flags {flags.value:#x})"
            streams.append(torch.cuda.ExternalStream(h.value))
        yield streams
    finally:
        torch.cuda.synchronize()
        for h in handles:
            hip().hipStreamDestroy(h)


class Blocker:
    """A chain of in-place elementwise torch ops over one large tensor, enqueued on a chosen stream, with an event behind it.
    The duration of one op is measured once with a pair of timing events: that times the torch op, not the code under test."""

    def __init__(self, torch):
        self.torch = torch
        self.x = torch.zeros(BLOCKER_ELEMENTS, dtype=torch.float32, device="cuda")
        for _ in range(4):
            self.x.add_(1.0)
        torch.cuda.synchronize()
        n = 32
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(n):
            self.x.add_(1.0)
        t1.record()
        t1.synchronize()
        self.ms_per_op = t0.elapsed_time(t1) / n
        assert self.ms_per_op > 0.0
        print(f"stream-order blocker: {self.ms_per_op:.4f} ms per op over {BLOCKER_ELEMENTS} float32 "
              f"({2 * 4 * BLOCKER_ELEMENTS / self.ms_per_op / 1e9:.2f} TB/s)")

    def enqueue(self, stream, ms):
        """About `ms` milliseconds of device work on `stream` (None: the null stream); returns the event behind it."""
        torch = self.torch
        stream = torch.cuda.default_stream() if stream is None else stream
        ops = max(1, math.ceil(ms / self.ms_per_op))
        with torch.cuda.stream(stream):
            for _ in range(ops):
                self.x.add_(1.0)
            done = torch.cuda.Event()
            done.record()
        return done


# ---------------------------------------------------------------------------
# content that reaches the device in stream order
# ---------------------------------------------------------------------------
def staged_tensor(torch, array):
    """A device copy of a numpy array, made before the blocker (a pageable upload may wait for the stream)."""
    import numpy as np

    return torch.from_numpy(np.ascontiguousarray(array).copy()).cuda()


def stage_image(im):
    """A tests/padded_images.PaddedImage whose host copy is final: keep that content in a staging tensor and leave zeros in
    the device buffer the pass will see, until write_image() has run in stream order."""
    torch = im.torch
    im.staged = torch.from_numpy(im.host.copy()).cuda()
    im.device = torch.zeros_like(im.staged)
    return im


def write_image(im):
    """Stream order: the staged content (sentinels and what write_inside() put there) into the live buffer."""
    im.device.copy_(im.staged)


def stage_scene(scene):
    for im in scene.images().values():
        stage_image(im)
    return scene


def write_scene(scene):
    for im in scene.images().values():
        write_image(im)


def copy2d_async(stream, image, source):
    """Stream order: rows of the uint8 device tensor `source` [h, row_bytes] into an abi.Image the library owns."""
    h, row_bytes = source.shape
    assert h <= image.height and row_bytes <= image.pitch_bytes and source.is_contiguous()
    rc = hip().hipMemcpy2DAsync(image.data, image.pitch_bytes, source.data_ptr(), row_bytes, row_bytes, h,
                                HIP_MEMCPY_DEVICE_TO_DEVICE, C.c_void_p(stream.cuda_stream))
    assert rc == 0, f"hipMemcpy2DAsync failed: {rc}"


GBUFFER_FIELDS = ("diffuse", "specular", "normal", "worldPosition", "occlusionRoughnessMetallic")


def stage_planes(torch, planes):
    """{field: [h, w, 4] array} of a G-buffer -> {field: uint8 device tensor [h, row bytes]}."""
    import numpy as np

    out = {}
    for name in GBUFFER_FIELDS:
        a = np.ascontiguousarray(planes[name])
        out[name] = torch.from_numpy(a.view(np.uint8).reshape(a.shape[0], -1).copy()).cuda()
    return out


def write_planes(stream, gbuffer, staged):
    """Stream order: staged planes into the five images of a szg_gbuffer (the planes a deferred pipeline owns)."""
    for name in GBUFFER_FIELDS:
        copy2d_async(stream, getattr(gbuffer, name), staged[name])


# ---------------------------------------------------------------------------
# the two arrangements
# ---------------------------------------------------------------------------
VARIANTS = ((0, "warm"), (1, "behind"), (2, "beside"))


def run_case(gpu, case):
    """Warm run, then behind and beside a blocker, all on one non-blocking stream and the same pipeline objects. Prints the
    blocker length and the observed margins; returns them.

    Everything a case made is released BEFORE the stream is destroyed: torch's pinned-memory allocator remembers the streams
    a pinned block was copied from (TStagedBuffer's ring, non_blocking copies) and records an event on each of them when the
    block is freed - on a destroyed stream that is a use after free inside the HIP runtime. A failing case would keep its
    frames, and with them those blocks, alive in the traceback: its error is therefore kept as text, the traceback dropped,
    and the failure raised again once the stream is gone."""
    failure = None
    with side_streams(gpu.torch, 1) as (S,):
        try:
            report = _run_case(gpu, case, S)
        except Exception as e:
            failure = failure_text(e)
        gc.collect()
        gpu.torch.cuda.synchronize()
    if failure is not None:
        pytest.fail(failure, pytrace=False)
    print("stream-order " + " ".join(f"{k}={v:.2f}" if isinstance(v, float) else f"{k}={v}" for k, v in report.items()))
    return report


def failure_text(e):
    """The error of a case with the traceback as text: nothing in it refers to a frame."""
    return "".join(traceback.format_exception(type(e), e, e.__traceback__))


def _run_case(gpu, case, S):
    torch, blocker = gpu.torch, gpu.blocker
    conditions = getattr(case, "conditions", True)
    report = {"case": case.id}
    state = case.setup(gpu)
    keep = []  # every run's buffers stay alive until the case ends
    try:
        run = case.prepare(gpu, state, 0)
        keep.append(run)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.cuda.stream(S):
            case.enqueue(gpu, state, run, S)
        host_s = time.perf_counter() - t0
        S.synchronize()
        total_s = time.perf_counter() - t0
        case.check(gpu, state, run, f"{case.id}, warm run on the side stream")
        ms = blocker_length_ms(host_s, total_s)
        report.update(warm_host_ms=host_s * 1e3, warm_total_ms=total_s * 1e3, blocker_ms=ms)

        # behind
        run = case.prepare(gpu, state, 1)
        keep.append(run)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        done = blocker.enqueue(S, ms)
        with torch.cuda.stream(S):
            case.enqueue(gpu, state, run, S)
        pending = not done.query()
        returned_s = time.perf_counter() - t0
        done.synchronize()
        report["behind_returned_ms"] = returned_s * 1e3
        report["behind_blocker_end_ms"] = (time.perf_counter() - t0) * 1e3
        S.synchronize()
        if conditions:
            assert pending, (f"{case.id}: inconclusive: blocker ended before the last record call returned "
                             f"({ms:.1f} ms blocker, the calls took {returned_s * 1e3:.2f} ms)")
        case.check(gpu, state, run, f"{case.id}, behind a blocker on its own stream")

        # beside
        run = case.prepare(gpu, state, 2)
        keep.append(run)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        done = blocker.enqueue(None, ms)
        with torch.cuda.stream(S):
            case.enqueue(gpu, state, run, S)
        S.synchronize()
        pending = not done.query()
        synced_s = time.perf_counter() - t0
        done.synchronize()
        report["beside_synced_ms"] = synced_s * 1e3
        report["beside_blocker_end_ms"] = (time.perf_counter() - t0) * 1e3
        assert pending, (f"{case.id}: inconclusive: blocker ended before S.synchronize() returned "
                         f"({ms:.1f} ms blocker on the null stream, the case took {synced_s * 1e3:.2f} ms)")
        case.check(gpu, state, run, f"{case.id}, beside a blocker on the null stream")
        torch.cuda.synchronize()
    finally:
        torch.cuda.synchronize()
        case.teardown(gpu, state)
        del keep
    return report


# ---------------------------------------------------------------------------
# frames in flight: several runs of one case behind ONE blocker, no host sync in between
# ---------------------------------------------------------------------------
def run_sequence(gpu, case, frames, conditions):
    """A warm run (variant 0), then `frames` runs (variants 1 ..) of `case` recorded back to back on one non-blocking
    stream behind one blocker, each into its own targets; then one S.synchronize() and every run is checked against its
    own expected result. case.restage(gpu, state, run) is called in front of every enqueue: the host-side staging of
    pipeline buffers that the next frame overwrites. `conditions`: assert condition A (False where the sequence needs
    more uploads than a staging ring has slots, or grows a buffer: a record call then waits by design)."""
    failure = None
    with side_streams(gpu.torch, 1) as (S,):
        try:
            report = _run_sequence(gpu, case, frames, conditions, S)
        except Exception as e:
            failure = failure_text(e)
        gc.collect()
        gpu.torch.cuda.synchronize()
    if failure is not None:
        pytest.fail(failure, pytrace=False)
    print("stream-order " + " ".join(f"{k}={v:.2f}" if isinstance(v, float) else f"{k}={v}" for k, v in report.items()))
    return report


def _run_sequence(gpu, case, frames, conditions, S):
    torch = gpu.torch
    report = {"sequence": case.id, "frames": frames}
    state = case.setup(gpu)
    try:
        warm = case.prepare(gpu, state, 0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.cuda.stream(S):
            case.restage(gpu, state, warm)
            case.enqueue(gpu, state, warm, S)
        host_s = time.perf_counter() - t0
        S.synchronize()
        total_s = time.perf_counter() - t0
        case.check(gpu, state, warm, f"{case.id}, warm run on the side stream")
        ms = blocker_length_ms(host_s * frames, total_s * frames)
        report.update(warm_host_ms=host_s * 1e3, warm_total_ms=total_s * 1e3, blocker_ms=ms)

        runs = [case.prepare(gpu, state, 1 + k) for k in range(frames)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        done = gpu.blocker.enqueue(S, ms)
        with torch.cuda.stream(S):
            for run in runs:
                case.restage(gpu, state, run)
                case.enqueue(gpu, state, run, S)
        pending = not done.query()
        returned_s = time.perf_counter() - t0
        done.synchronize()
        report["behind_returned_ms"] = returned_s * 1e3
        report["behind_blocker_end_ms"] = (time.perf_counter() - t0) * 1e3
        report["pending_at_return"] = pending
        S.synchronize()
        if conditions:
            assert pending, (f"{case.id}: inconclusive: blocker ended before the last record call returned "
                             f"({ms:.1f} ms blocker, the calls took {returned_s * 1e3:.2f} ms)")
        for k, run in enumerate(runs):
            run.last = k == frames - 1  # state the pipeline owns (G-buffer planes, shadow maps) holds the last frame only
            case.check(gpu, state, run, f"{case.id}, frame {k + 1} of {frames} in flight behind a blocker")
    finally:
        torch.cuda.synchronize()
        case.teardown(gpu, state)
    return report
