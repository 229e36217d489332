"""Stream-ordering harness of tests/test_gpu_stream_ordering.py and tests/loopback/worker_stream.py (a plain module, no fixtures).

include/bp5.h promises that every call enqueues on the handle's stream.  On the null stream a launch, fill or copy that went to the wrong
stream still runs in order, and so does a legacy hipMemcpy without a synchronisation in front of it.  Here the handle sits on a NON-BLOCKING
side stream S (torch's pool streams are: they do not synchronise with the null stream) that is kept busy:

  hold(S)      a bounded spin on S (a few tens of milliseconds) and an event recorded right behind it;
  producers    torch copies, enqueued on S behind the spin, that bring the good inputs into working tensors which hold NaN until then;
  the call     made while held(ev) is still true: whatever it enqueues is enqueued while its inputs are NaN;
  consumer     out = dst.clone() on S, no host synchronisation in between.

Work the library put on another stream runs ahead of the producers and reads NaN, or is overwritten by them; a host value copied back without a
synchronisation of S is computed from NaN.  run() is the protocol of one case."""
import numpy as np
import torch

HOLD_MS = 40.0          # length of one hold: long against the host time of a warmed call (tens of microseconds), short for the suite
SENTINEL = -7.25e30     # padding of block vectors, content of an output before its producer ran (tests/test_gpu_elasticity.py)
_state = {}


def side_stream():
    """a fresh non-blocking stream"""
    return torch.cuda.Stream()


def _elapsed_ms(stream, work):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        a.record(stream)
        work()
        b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def _matmul_chain(n):
    m = _state["matrix"]
    for _ in range(n):
        torch.mm(m, m, out=_state["product"])


def calibrate():
    """once per process: how many _sleep cycles (or, where _sleep does not delay on this device, how many FP64 matmuls) make HOLD_MS"""
    if _state:
        return _state
    s = side_stream()
    probe = 20_000_000
    _elapsed_ms(s, lambda: torch.cuda._sleep(1000))                  # (loads the kernel)
    ms = _elapsed_ms(s, lambda: torch.cuda._sleep(probe))
    if ms >= 1.0:
        _state.update(kind="sleep", cycles=int(probe * HOLD_MS / ms), probe_ms=ms)
    else:
        with torch.cuda.stream(s):
            _state["matrix"] = torch.eye(768, dtype=torch.float64, device="cuda")
            _state["product"] = torch.empty_like(_state["matrix"])
        _elapsed_ms(s, lambda: _matmul_chain(2))
        ms = _elapsed_ms(s, lambda: _matmul_chain(20))
        _state.update(kind="matmul", count=max(1, int(20 * HOLD_MS / ms)), probe_ms=ms)
    # the torch kernels of the producers and the consumer, loaded before any hold
    with torch.cuda.stream(s):
        t = torch.zeros(8, dtype=torch.float64, device="cuda")
        t.fill_(float("nan"))
        t.copy_(torch.ones_like(t))
        t.clone()
    s.synchronize()
    _state["measured_ms"] = _elapsed_ms(s, lambda: _spin(1.0))
    print(f"stream harness: hold by {_state['kind']}, {_state.get('cycles', _state.get('count'))} units, measured {_state['measured_ms']:.1f} ms")
    return _state


def _spin(scale):
    st = _state
    if st["kind"] == "sleep":
        torch.cuda._sleep(int(st["cycles"] * scale))
    else:
        _matmul_chain(max(1, int(st["count"] * scale)))


def hold(stream, scale=1.0):
    """enqueue scale * HOLD_MS of spinning on `stream`; the event recorded right behind it"""
    calibrate()
    ev = torch.cuda.Event()
    with torch.cuda.stream(stream):
        _spin(scale)
        ev.record(stream)
    return ev


def held(ev):
    return not ev.query()


def on_device(a):
    """a numpy array as a float64 tensor on the CURRENT stream's device"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:0")


def run(S, inputs, outputs, call, asynchronous=False, hold_null=False, scale=1.0):
    """One case.  inputs: [(working tensor, staging tensor with the good values)]; outputs: [(tensor, staging tensor with its pre-content, or None:
    NaN)]; call(): the library call, reading and writing the working tensors.  asynchronous: the entry point is documented as such, the call is a
    warmed one -- it must return while the hold still lasts.  scale: the hold is that many HOLD_MS long.  hold_null: the null stream is held as well, twice as long.  A host-synchronous
    entry point may wait for its stream before it enqueues anything (the solvers do); from then on its stream is idle, and a launch that went
    to the null stream would merely race with the ones behind it.  Behind a held null stream it comes late for certain, and the launches that
    follow on the handle's stream run without it.  (A synchronisation that waits for the wrong stream shows WITHOUT this second hold, which is why
    the solver cases run once each way.)  Returns (clones of the outputs taken on S, what call() returned); the inputs are
    checked to be unchanged."""
    with torch.cuda.stream(S):
        torch.cuda.synchronize()
        for w, _ in inputs:                                    # poison
            w.fill_(float("nan"))
        for o, _ in outputs:
            o.fill_(SENTINEL)
        torch.cuda.synchronize()
        ev = hold(S, scale)
        if hold_null:
            hold(torch.cuda.default_stream(), 2.0 * scale)
        for w, good in inputs:                                 # producers, behind the hold
            w.copy_(good)
        for o, pre in outputs:
            o.fill_(float("nan")) if pre is None else o.copy_(pre)
        assert held(ev), "the hold ended before the call was made: nothing is tested"
        value = call()
        if asynchronous:
            assert held(ev), "an asynchronous entry point waited for the stream (or the hold is too short for the host time of the call)"
        got = [o.clone() for o, _ in outputs]                  # consumer, no host synchronisation
        S.synchronize()
        for w, good in inputs:
            assert torch.equal(torch.nan_to_num(w, nan=1.25e300), torch.nan_to_num(good, nan=1.25e300)), "an input was changed"
    return got, value
