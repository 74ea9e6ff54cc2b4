"""The measurement method of the tools/time_*.py scripts, decode_bench.py and event_overhead.py, stated once (`import timing`).

Method.  Everything a contender touches is allocated first.  Every contender is warmed (`warm`: for some seconds or some calls, the
policy each tool's profile was recorded with).  Then the contenders alternate round by round (`alternate`), in one process or -- where
two source trees or two module states cannot share a process -- in one child process per side (`Child`, `serve`), only one of them
running at a time.  One timing is a pair of device events around back-to-back calls with no host synchronisation between them
(`event_time`, ms per call; the caller scales to its unit).  Reported are the median with min and max over the rounds (`stats`,
`values_and_stats`), and a contender runs a second time under another name in every round ("dense-2", "base-2", "parent-2"), which
shows the spread of a contender against itself.  Two sets of timings are called apart only when their ranges do not overlap (`apart`).
The scripts that print one figure per line warm some calls and time once (`one_shot`).

The rest is what the tools' set-up shares: the log behind --out (`Log`), the device header line, a graph replay from a side-stream
capture (`graphed`), another build of the library typed from this tree's signature table (`load_library`), pre-bound ctypes calls
(`bound`), and the packed stateful inference batch of the time_rwkv6_* tools (`packed_batch`, `dense_calls`).

Importing this module does not import torch: the parents of the child-process tools never open the GPU.
"""
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

median = statistics.median
TAG = "@@ "                                                  # a line of a child's stdout that carries a JSON record


# ---- the log and the header
class Log:
    """say() prints and collects; write(path) leaves the collected lines in the file, or nothing when there is no path."""

    def __init__(self):
        self.lines = []

    def say(self, s=""):
        print(s, flush=True)
        self.lines.append(s)

    def write(self, path):
        if path:
            with open(path, "w") as fh:
                fh.write("\n".join(self.lines) + "\n")


def device_record():
    """What a child process says of its device in its hello record."""
    import torch
    p = torch.cuda.get_device_properties(0)
    return {"device": p.name, "cus": p.multi_processor_count, "torch": torch.__version__, "hip": torch.version.hip}


def device_header(record=None):
    """The header line, of this process's device or of a child's hello record."""
    h = record or device_record()
    return f"device: {h['device']}, {h['cus']} CUs; torch {h['torch']}; hip {h['hip']}"


# ---- one timing
def event_time(fn, iters):
    """ms per call of `iters` back-to-back calls, between two device events"""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def warm(fn, seconds=None, calls=None, sync="end"):
    """Call fn for `seconds`, or `calls` times; synchronise after "each" call, once at the "end", or not at all (None)."""
    import torch
    t0, n = time.time(), 0
    while n < calls if seconds is None else time.time() - t0 < seconds:
        fn()
        n += 1
        if sync == "each":
            torch.cuda.synchronize()
    if sync == "end":
        torch.cuda.synchronize()


def one_shot(fn, iters, warm_calls):
    """warm some calls, synchronise, time once: ms per call"""
    warm(fn, calls=warm_calls)
    return event_time(fn, iters)


def phase_times(fwd, bwd, iters):
    """A (forward, backward) contender's turn in a round: one forward, so that the backward finds its checkpoints, then ms per call of
    the forward, of the backward and of the step"""
    fwd()
    return event_time(fwd, iters), event_time(bwd, iters), event_time(lambda: (fwd(), bwd()), iters)


def alternate(contenders, measure, repeats, before=None):
    """{name: [measure(contender), one per round]}: every round takes the contenders in their order; before() runs in front of each"""
    res = {name: [] for name in contenders}
    for _ in range(repeats):
        for name, c in contenders.items():
            if before:
                before()
            res[name].append(measure(c))
    return res


# ---- what is said of a list of timings
def stats(xs, width, prec):
    return f"median {median(xs):{width}.{prec}f}  min {min(xs):{width}.{prec}f}  max {max(xs):{width}.{prec}f}"


def values_and_stats(xs, width, prec):
    return " ".join(f"{x:{width}.{prec}f}" for x in xs) + "   " + stats(xs, width, prec)


def apart(a, b):
    """True when the ranges of the two lists do not overlap; ranges that touch overlap"""
    return max(a) < min(b) or min(a) > max(b)


# ---- graph replay
def graphed(fn):
    """(replay, what fn returned under capture): fn run once on a side stream, then captured there"""
    import torch
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            kept = fn()
    torch.cuda.current_stream().wait_stream(side)
    return g.replay, kept


# ---- one side per child process: JSON records on tagged lines of stdout, questions as JSON lines on stdin
def emit(record):
    print(TAG + json.dumps(record), flush=True)


def records(text):
    return [json.loads(line[len(TAG):]) for line in text.splitlines() if line.startswith(TAG)]


class Child:
    """A fresh python process on `argv` (the tool's own file and its worker arguments) that runs serve()."""

    def __init__(self, argv, cwd):
        self.p = subprocess.Popen([sys.executable] + argv, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, cwd=cwd)
        self.hello = self.read()

    def read(self):
        for line in self.p.stdout:
            if line.startswith(TAG):
                r = json.loads(line[len(TAG):])
                if "error" in r:
                    raise RuntimeError(r["error"])
                return r
        raise RuntimeError(f"the child process ended (exit code {self.p.wait()})")

    def ask(self, **q):
        self.p.stdin.write(json.dumps(q) + "\n")
        self.p.stdin.flush()
        return self.read()

    def close(self):
        try:
            self.p.stdin.write(json.dumps({"op": "quit"}) + "\n")
            self.p.stdin.close()
        except OSError:
            pass
        self.p.wait()


def serve(hello, ops):
    """The worker's loop: the hello record, then one reply per question {"op": name, **arguments} from ops[name](**arguments), until
    "quit" or the end of stdin.  An exception is the reply {"error": ...}: reported, not hidden -- the parent raises it and stops."""
    emit(hello)
    for line in sys.stdin:
        q = json.loads(line)
        op = q.pop("op")
        if op == "quit":
            break
        try:
            if op not in ops:
                raise ValueError(op)
            r = ops[op](**q) or {}
        except Exception as e:
            r = {"error": f"{type(e).__name__}: {e}"}
        emit(r)


# ---- raw library calls
def load_library(path, signatures, lacks=None):
    """Another build of the library with the calls of `signatures` ({symbol: (restype, argtypes)}, from rwkv_lm_ext_amd/_lib.py) typed;
    lacks = (symbol, what it is): refuse a build that already has it, which is then not the parent commit's"""
    h = ctypes.CDLL(os.path.abspath(path))
    for name, (res, args) in signatures.items():
        fn = getattr(h, name)
        fn.restype, fn.argtypes = res, args
    if lacks:
        assert not hasattr(h, lacks[0]), f"--parent-lib already has {lacks[1]}: not the parent commit's library"
    return h


def bound(fn, *args):
    """fn(*args) with its arguments bound once; every call asserts that the library returned 0"""
    def run():
        rc = fn(*args)
        assert rc == 0, rc
    return run


# ---- the packed stateful inference batch (time_rwkv6_varlen.py, time_rwkv6_split.py)
def packed_batch(lens, H, g, ws_bytes):
    """bf16 r, k, v, y [total, C], fp32 decay w, cu_seqlens, a zero state pool of one slot per sequence and a caller workspace"""
    import torch
    total, C = sum(lens), 64 * H
    r, k, v = (torch.randn(total, C, device="cuda", generator=g).mul_(0.5).to(torch.bfloat16) for _ in range(3))
    w = torch.exp(-torch.exp(torch.randn(total, C, device="cuda", generator=g) - 2.0)).contiguous()
    y = torch.empty(total, C, device="cuda", dtype=torch.bfloat16)
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32, device="cuda")
    pool = torch.zeros(len(lens), H, 64, 64, device="cuda")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    return dict(r=r, k=k, v=v, w=w, y=y, cu=cu, pool=pool, ws=ws, lens=lens, total=total)


def dense_calls(fn, d, rows, H, u, stream):
    """The loop of dense rwkv6_cuda_forward_bf16 calls (fn) over a packed batch; rows: (first token, B, T, first slot) per call"""
    C, p = 64 * H, lambda t: t.data_ptr()
    calls = []
    for t0, B, T, slot in rows:
        el = t0 * C
        calls.append((B, T, C, H, p(d["pool"]) + slot * H * 4096 * 4, p(d["r"]) + el * 2, p(d["k"]) + el * 2, p(d["v"]) + el * 2,
                      p(d["w"]) + el * 4, p(u), p(d["y"]) + el * 2, stream))

    def run():
        for args in calls:
            rc = fn(*args)
            assert rc == 0, rc
    return run
