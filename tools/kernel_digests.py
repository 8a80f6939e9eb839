"""The device code of every translation unit of kajo_amd/csrc as a digest per function, for "this change moved no kernel but its own".

    python tools/kernel_digests.py [--csrc DIR] [--leave-out UNIT ...] > tests/golden/kernel_digests_<what>.json

Every `.hip` unit `make all` compiles is compiled by the Makefile's own command (`make -n`), with the device assembly asked for instead of
an object (-S --cuda-device-only). A function is the text from its label to its `.Lfunc_end`: every instruction of every exit, not only
those in front of the first s_endpgm. Comments and blank lines are dropped and the unit's function index is taken out of the local
labels (.LBB12_3 -> .LBB_3), so that a function another one was put in front of keeps its digest; nothing else is normalised: an
instruction, a register, an operand, a label or an alignment that differs gives another SHA-256.

--csrc DIR reads another tree's kajo_amd/csrc (a `git worktree` of the commit to record from). tests/test_noise_cpu.py compares the
working tree against tests/golden/kernel_digests_before_noise.json, recorded with this tool from the commit in front of the noise
estimate (--leave-out nothing: noise.hip did not exist). A change that means to move a kernel records the file again, from its own parent
commit, and says so."""
import argparse
import concurrent.futures
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def compiler():
    out = subprocess.run(["hipcc", "--version"], capture_output=True, text=True).stdout
    return " | ".join(l.strip() for l in out.splitlines() if re.match(r"(HIP version|AMD clang version)", l))


def units(csrc):
    """unit name -> the Makefile's compile command of every device translation unit, as a list"""
    plan = subprocess.run(["make", "-n", "-B", "-C", csrc, "all"], capture_output=True, text=True, check=True).stdout
    found = {}
    for line in plan.splitlines():
        cmd = line.split()
        src = [w for w in cmd if w.endswith(".hip")]
        if line.startswith("hipcc") and "-c" in cmd and len(src) == 1 and any(w.startswith("--offload-arch=") for w in cmd):
            found[os.path.basename(src[0])[:-len(".hip")]] = cmd
    return found


def assembly(cmd):
    """the device assembly the command's flags give"""
    with tempfile.TemporaryDirectory(prefix="kajo_digest_") as tmp:
        asm = os.path.join(tmp, "k.s")
        i = cmd.index("-c")
        cmd = cmd[:i] + ["-S", "--cuda-device-only"] + cmd[i + 1:]
        cmd[cmd.index("-o") + 1] = asm
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode:
            raise RuntimeError(r.stderr[-3000:])
        return open(asm).read()


def functions(asm):
    """function name -> its normalised text, label to .Lfunc_end"""
    found = {}
    for name in re.findall(r"^\s*\.type\s+([\w.$]+),@function", asm, re.M):
        start = asm.index("\n" + name + ":")
        body = asm[start + 1:asm.index(".Lfunc_end", start)]
        lines = (re.sub(r"\.LBB\d+_", ".LBB_", l.split(";")[0]).strip() for l in body.splitlines())
        found[name] = "\n".join(l for l in lines if l)
    return found


def digests(csrc, leave_out=()):
    """unit -> {function: SHA-256 of its normalised text}, the units compiled side by side"""
    cmds = {u: c for u, c in units(csrc).items() if u not in leave_out}
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        texts = dict(zip(cmds, pool.map(assembly, cmds.values())))
    return {u: {f: hashlib.sha256(t.encode()).hexdigest() for f, t in sorted(functions(texts[u]).items())} for u in sorted(texts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--csrc", default=os.path.join(ROOT, "kajo_amd", "csrc"))
    ap.add_argument("--leave-out", nargs="*", default=[])
    args = ap.parse_args()
    json.dump({"compiler": compiler(), "units": digests(os.path.abspath(args.csrc), args.leave_out)}, sys.stdout, indent=1, sort_keys=True)
    sys.stdout.write("\n")


if __name__ == "__main__":
    main()
