"""What the compiler makes of a device translation unit of kajo_amd/csrc, for the tests that pin kernels without a GPU (hipcc
cross-compiles gfx950): the Makefile's own compile command (`make -n`), run with the device assembly and the resource remarks asked for
instead of an object file, once per session and unit. Each test file keeps its own kernel lists, budgets and instruction-mix
assertions; this module holds only the plumbing they shared. Beside it: tools/kernel_digests.py, loaded once, and its digests of the
working tree, computed once."""
import collections
import functools
import importlib.util
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kajo_amd", "csrc")

# cmd: the Makefile's own argv; resources: {function: {remark key: int}}; asm: the device assembly of the unit
Built = collections.namedtuple("Built", "cmd resources asm")
_BUILT = {}


def need_tools():
    if shutil.which("hipcc") is None or shutil.which("make") is None:
        pytest.skip("hipcc / make not available")


@functools.lru_cache(maxsize=None)
def _plan():
    return subprocess.run(["make", "-n", "-B", "-C", CSRC, "all"], capture_output=True, text=True, check=True).stdout


def compile_command(source, plan=None):
    """argv of the one `hipcc ... -c` line of `make all`'s plan that names /<source> (glare.hip, kernel_exact.hip, checkpoint_kernels.cpp)"""
    lines = [l for l in (_plan() if plan is None else plan).splitlines()
             if l.startswith("hipcc") and "-c" in l.split() and any(w.endswith("/" + source) for w in l.split())]
    assert len(lines) == 1, "%s: %d compile lines name it: %s" % (source, len(lines), lines)
    return lines[0].split()


def parse_remarks(stderr_text):
    """-Rpass-analysis=kernel-resource-usage remarks -> {function: {key: int}}; a key is the text in front of " [": VGPRs, AGPRs,
    SGPRs Spill, VGPRs Spill, ScratchSize, Occupancy, LDS Size and every other numeric one"""
    res, name = {}, None
    for line in stderr_text.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            res[name] = {}
            continue
        m = re.search(r"remark:\s+([^:]+): (\d+)\b", line)
        if m and name:
            res[name][m.group(1).split(" [")[0]] = int(m.group(2))
    return res


def build(source):
    """Built(cmd, resources, asm) of the unit, compiled as the Makefile compiles it (device code only); the same object every time"""
    need_tools()
    cmd = compile_command(source)
    if tuple(cmd) not in _BUILT:
        with tempfile.TemporaryDirectory(prefix="kajo_devicecode_") as tmp:
            asm = os.path.join(tmp, "k.s")
            i = cmd.index("-c")
            run = cmd[:i] + ["-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"] + cmd[i + 1:]
            run[run.index("-o") + 1] = asm
            r = subprocess.run(run, capture_output=True, text=True)
            assert r.returncode == 0, r.stderr[-3000:]
            _BUILT[tuple(cmd)] = Built(cmd, parse_remarks(r.stderr), open(asm).read())
    return _BUILT[tuple(cmd)]


def body(asm, kernel, end="s_endpgm"):
    """the kernel's text from its label to the first `end` behind it (s_endpgm: its first exit; .Lfunc_end: every exit)"""
    text = asm[asm.index("\n" + kernel + ":"):]
    return text[:text.index(end)]


@functools.lru_cache(maxsize=None)
def digest_tool():
    spec = importlib.util.spec_from_file_location("kernel_digests", os.path.join(ROOT, "tools", "kernel_digests.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


@functools.lru_cache(maxsize=None)
def _digests():
    return digest_tool().digests(CSRC)


def digests_now():
    """unit -> {function: digest} of the working tree, by tools/kernel_digests.py; a copy: the caller may take it apart"""
    need_tools()
    return {unit: dict(functions) for unit, functions in _digests().items()}
