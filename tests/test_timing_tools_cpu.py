"""tools/timing.py, the measurement harness of the tools/time_*.py scripts, without a GPU: the summary and the overlap verdict, the log's
bytes, the child-process protocol against a fake worker, no torch at import, and every converted script still starting (--help)."""
import glob
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
sys.path.insert(0, TOOLS)

import timing          # noqa: E402


def test_summary_of_a_list():
    xs = [3.0, 1.0, 10.0, 2.0]                                      # median of an even count: the mean of the middle two
    assert timing.median(xs) == 2.5
    assert timing.stats(xs, 8, 1) == "median      2.5  min      1.0  max     10.0"
    assert timing.values_and_stats(xs, 8, 1) == "     3.0      1.0     10.0      2.0   median      2.5  min      1.0  max     10.0"
    assert timing.values_and_stats((0.1234, 0.5), 7, 3) == "  0.123   0.500   median   0.312  min   0.123  max   0.500"


def test_ranges_are_apart_only_with_a_gap():
    assert timing.apart([1.0, 2.0], [2.5, 3.0]) and timing.apart([2.5, 3.0], [1.0, 2.0])
    assert not timing.apart([1.0, 2.0], [2.0, 3.0]) and not timing.apart([2.0, 3.0], [1.0, 2.0])      # touching ranges overlap
    assert not timing.apart([1.0, 3.0], [2.0, 2.5]) and not timing.apart([2.0, 2.5], [1.0, 3.0])      # one inside the other
    assert not timing.apart([1.0], [1.0])
    assert timing.apart([5.0, 4.0], (1.0, 3.0))                                                       # against a (lo, hi) pair


def test_alternate_takes_the_contenders_in_order_every_round():
    seen = []
    res = timing.alternate({"a": 1, "b": 2}, lambda c: seen.append(c) or 10 * c, 3, before=lambda: seen.append("before"))
    assert res == {"a": [10, 10, 10], "b": [20, 20, 20]}
    assert seen == ["before", 1, "before", 2] * 3
    assert timing.alternate({"a": 1}, lambda c: c, 2) == {"a": [1, 1]}


def test_warm_by_calls_and_by_seconds():
    calls = []
    timing.warm(lambda: calls.append(1), calls=7, sync=None)        # (sync=None: no device call, so this runs without a GPU)
    assert len(calls) == 7
    del calls[:]
    timing.warm(lambda: calls.append(1), seconds=0.01, sync=None)
    assert calls
    del calls[:]
    timing.warm(lambda: calls.append(1), seconds=0.0, sync=None)
    assert not calls


def test_log_writes_its_lines_and_one_newline(tmp_path, capsys):
    log = timing.Log()
    log.say("first")
    log.say()
    log.say("third")
    assert capsys.readouterr().out == "first\n\nthird\n"
    out = tmp_path / "out.txt"
    log.write(str(out))
    assert out.read_bytes() == b"first\n\nthird\n"
    before = set(os.listdir(tmp_path))
    log.write(None)                                                 # no --out: no file
    assert set(os.listdir(tmp_path)) == before


def test_device_header_from_a_hello_record():
    hello = {"ready": True, "device": "AMD Instinct MI355X", "cus": 256, "torch": "2.9", "hip": "7.0"}
    assert timing.device_header(hello) == "device: AMD Instinct MI355X, 256 CUs; torch 2.9; hip 7.0"


FAKE_WORKER = """
import sys
sys.path.insert(0, sys.argv[1])
import timing
def fail(): raise KeyError("no such case")
print("a line of the worker's own that carries no record")
timing.serve({"ready": True}, {"double": lambda x: {"x": 2 * x}, "nothing": lambda: None, "fail": fail, "leave": lambda: sys.exit(3)})
"""


def test_child_protocol_against_a_fake_worker(tmp_path):
    kid = timing.Child(["-c", FAKE_WORKER, TOOLS], cwd=str(tmp_path))
    try:
        assert kid.hello == {"ready": True}
        assert kid.ask(op="double", x=21) == {"x": 42}
        assert kid.ask(op="nothing") == {}
        with pytest.raises(RuntimeError, match="KeyError: 'no such case'"):
            kid.ask(op="fail")
        with pytest.raises(RuntimeError, match="ValueError: unknown"):
            kid.ask(op="unknown")
        assert kid.ask(op="double", x=1) == {"x": 2}                # an error reply does not end the worker
        with pytest.raises(RuntimeError, match=r"the child process ended \(exit code 3\)"):
            kid.ask(op="leave")
    finally:
        kid.close()
    kid = timing.Child(["-c", FAKE_WORKER, TOOLS], cwd=str(tmp_path))
    kid.close()                                                     # "quit" ends the loop
    assert kid.p.returncode == 0


def test_records_are_the_tagged_lines():
    text = "noise\n" + timing.TAG + '{"a": 1}\nmore noise\n' + timing.TAG + '{"done": true}\n'
    assert timing.records(text) == [{"a": 1}, {"done": True}]


def run(*argv):
    return subprocess.run([sys.executable, *argv], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def test_importing_the_module_does_not_import_torch():
    r = run("-c", f"import sys; sys.path.insert(0, {TOOLS!r}); import timing; assert 'torch' not in sys.modules, 'torch was imported'")
    assert r.returncode == 0, r.stdout


CONVERTED = sorted(os.path.basename(p) for p in glob.glob(os.path.join(TOOLS, "time_*.py"))) + ["decode_bench.py", "event_overhead.py", "fwd_ab.py"]
WITH_PARSER = [name for name in CONVERTED if "argparse" in open(os.path.join(TOOLS, name)).read()]


def test_every_converted_tool_uses_the_module():
    assert len(CONVERTED) >= 20 and len(WITH_PARSER) >= 14          # (a new time_*.py joins both lists by itself)
    for name in CONVERTED:
        assert "import timing" in open(os.path.join(TOOLS, name)).read(), name


@pytest.mark.parametrize("name", WITH_PARSER)
def test_help_exits_0(name):
    r = run(os.path.join(TOOLS, name), "--help")
    assert r.returncode == 0, r.stdout
    assert "usage:" in r.stdout


def test_scan_kernels_rehearsal():
    r = run(os.path.join(TOOLS, "time_scan_kernels.py"), "--dry", "--parent-lib", "none")
    assert r.returncode == 0, r.stdout
    assert "equality: " in r.stdout and "speed: 11 rows built" in r.stdout
