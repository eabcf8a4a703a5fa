#!/usr/bin/env python3
"""What the seven *_host_check.py scripts share: tools/stage_host.hip built once with AddressSanitizer and
UBSan on the host side (it includes api.hip, so it walks the library's own launch plan), a directory for
its files, one run of a sub-command, and the cleanup.  No GPU.

Every script takes  --keep  (leave the directory) and  --csrc DIR  (api.hip, scale.hip, kernels.hip and
sws_filter.cpp from DIR, a changed copy of ffmpeg_distributed_amd/csrc: the mutation runs of
profiles/host_plan/mutations.txt).  Several checks on one build:

usage: python3 tools/host_check.py [--keep] [--csrc DIR] CHECK[:FLAG] ...
       (CHECK: yadif, unsharp, lut, cmat, tile, hist, hqdn3d; FLAG: the script's --sweep or --long, e.g. yadif:--sweep)"""
import importlib
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
SHIFTS = {"420": (1, 1), "422": (1, 0), "444": (0, 0)}


class Host:
    def __init__(self, args):
        self.keep = "--keep" in args
        csrc = ([args[i + 1] for i, a in enumerate(args[:-1]) if a == "--csrc"] or [os.path.join(ROOT, "ffmpeg_distributed_amd", "csrc")])[0]
        self.tmp = tempfile.mkdtemp(prefix="stage_host_")
        self.exe = self.path("stage_host")
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                        "-Xarch_host", "-fno-omit-frame-pointer", "-Wno-pass-failed", "-I", os.path.join(ROOT, "include"),
                        "-I", csrc, "-o", self.exe, os.path.join(ROOT, "tools", "stage_host.hip"),
                        os.path.join(csrc, "sws_filter.cpp")], check=True)

    def path(self, name):
        return os.path.join(self.tmp, name)

    def run(self, stage, args, what):
        """One sub-command; `what` names the case when it fails (a sanitizer stop, an assertion, a refusal)."""
        r = subprocess.run([self.exe, stage] + [str(a) for a in args], capture_output=True, text=True)
        if r.returncode:
            sys.exit(f"stage_host {stage} failed ({r.returncode}) at {what}:\n" + r.stderr[-4000:])
        return r.stdout

    def close(self):
        if not self.keep:
            for f in os.listdir(self.tmp):
                os.unlink(self.path(f))
            os.rmdir(self.tmp)


def run_check(check, args=None, host=None):
    """A script's check(host, args) -> mismatches, on `host` or a build of its own; its last line and exit status."""
    args = sys.argv[1:] if args is None else args
    own = host is None
    host = host or Host(args)
    try:
        bad = check(host, args)
    finally:
        if own:
            host.close()
    print("all equal" if not bad else f"{bad} mismatches")
    return 1 if bad else 0


def split_arg(split):
    return ",".join(str(v) for v in split) if split else "0"


if __name__ == "__main__":
    host, rc = Host(sys.argv[1:]), 0
    try:
        for spec in [a for a in sys.argv[1:] if a.split(":")[0] in ("yadif", "unsharp", "lut", "cmat", "tile", "hist", "hqdn3d")]:
            name, _, flag = spec.partition(":")
            print(f"# {name}_host_check.py {flag}".rstrip(), flush=True)
            rc |= run_check(importlib.import_module(name + "_host_check").check, [flag] if flag else [], host)
    finally:
        host.close()
    sys.exit(rc)
