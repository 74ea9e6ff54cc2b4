"""The gfx950 device listing of a kernel source and the parsers the ISA guards share (tests/test_isa_cpu.py, tests/test_isa_spills_cpu.py,
tests/test_wkv5_cpu.py, tools/check_waitcnt.py, tools/issue_model.py, tools/issue_floor.py).  No GPU needed: hipcc cross-compiles.

The flags are the build's own (rwkv_lm_ext_amd/_build.py), so a guard reads the code that ships, and a source is compiled at most once
per process, however many guards read its listing.
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from rwkv_lm_ext_amd import _build                                  # noqa: E402

CSRC = _build.CSRC
COMPILED = []       # the compile log: the path of every source compiled by this process, in order
_listings = {}


class HipccMissing(RuntimeError):
    """hipcc is not on PATH: there is no listing to be had."""


def flags():
    """The build's flags without its warning switches, as an assembly listing of the device code alone."""
    return [f for f in _build.HIPCC_FLAGS if not f.startswith("-W")] + ["-w", "-S", "--cuda-device-only"]


def listing(src, csrc=CSRC, quiet=False):
    """The gfx950 listing of csrc/<src> as text (csrc: the source directory of another tree; quiet: hipcc's stderr is dropped, as the
    command-line tools always ran it)."""
    path = os.path.abspath(os.path.join(csrc, src))
    if path not in _listings:
        if shutil.which("hipcc") is None:
            raise HipccMissing("hipcc not on PATH")
        with tempfile.TemporaryDirectory() as tmp:
            out = os.path.join(tmp, src + ".s")
            subprocess.check_call(["hipcc"] + flags() + ["-o", out, path], stderr=subprocess.DEVNULL if quiet else None)
            with open(out) as f:
                _listings[path] = f.read()
        COMPILED.append(path)
    return _listings[path]


def kernel_meta(asm, key):
    """{kernel name: value} of one integer key of the kernels' metadata (vgpr_spill_count, private_segment_fixed_size, vgpr_count, ...)."""
    names = re.findall(r"^\s+\.name:\s+(\S+)", asm, re.M)
    vals = [int(x) for x in re.findall(r"^\s+\." + key + r":\s+(\d+)", asm, re.M)]
    assert len(names) == len(vals) and names
    return dict(zip(names, vals))


def functions(asm):
    """{mangled name: text} of every function `_Z...:` of a listing, in its order (a function's text runs up to the next one)."""
    return {f.split(":", 1)[0]: f for f in re.split(r"\n(?=_Z[\w]+:)", asm) if re.match(r"_Z\w+:", f)}


def function(asm, substr):
    """(name, text) of the first function whose name contains substr; none: the end of the program, as the tools always ended there."""
    for name, text in functions(asm).items():
        if substr in name:
            return name, text
    raise SystemExit(f"no function matching {substr}")


def blocks(fn):
    """The basic blocks of one function: (label, comment, lines) per `.LBBn_m:` label, label without its `.L`, lines up to the next label.
    comment is what the asm printer wrote on the label's line, '' if nothing: `; =>This Loop Header: Depth=n` on a loop's first block,
    `; in Loop: Header=BBn_m Depth=n` on its other blocks, `; Parent Loop BBn_m Depth=n` on the header of a loop inside another (its own
    `Inner Loop Header: Depth=n` follows on a comment line).  The lines in front of the first label come first, as label None."""
    label, comment, lines = None, "", []
    for line in fn.split("\n"):
        m = re.match(r"^\.L(BB\d+_\d+):\s*(;.*)?$", line)
        if m:
            yield label, comment, lines
            label, comment, lines = m.group(1), m.group(2) or "", []
        else:
            lines.append(line)
    yield label, comment, lines
