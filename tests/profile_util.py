"""Helpers shared by the tests that read `rocprofv3 --kernel-trace --stats` summaries (the committed ones under profiles/,
written by tools/save_profiles.py, and the ones tests/test_gpu_operating_points.py has a child process write)."""
import csv
import glob
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the newest set that tools/save_profiles.py committed
TAG = max((os.path.basename(p).split("_bench_")[0] for p in glob.glob(os.path.join(ROOT, "profiles", "r*_v*_bench_c3.json"))),
          key=lambda t: [int(v) for v in t.replace("r", "").replace("v", "").split("_")])


def _march_kernel_args(name):
    return [a.strip() for a in name[len("void march_kernel<"):].split(">")[0].split(",")]


def frame_march(name):
    """Is this kernel name a frame march: march_pool_kernel, or march_kernel<SPEC, RES, RECORD = false, LIST = false, ...>?"""
    if name.startswith("void march_pool_kernel<"):
        return True
    if not name.startswith("void march_kernel<"):
        return False
    args = _march_kernel_args(name)
    return args[2] == "false" and args[3] == "false"


def retrace_march(name):
    """Is this kernel name a re-trace launch of the frame: march_kernel<SPEC, RES, RECORD = false, LIST = true, ...>?"""
    if not name.startswith("void march_kernel<"):
        return False
    args = _march_kernel_args(name)
    return args[2] == "false" and args[3] == "true"


def kernel_stats_rows(path):
    return list(csv.DictReader(open(path)))


def committed_kernel_stats(cfg):
    """Rows of profiles/<TAG>_<cfg>_kernel_stats.csv (cfg: c2, c3, c5, c3_reseed, ...)."""
    return kernel_stats_rows(os.path.join(ROOT, "profiles", "%s_%s_kernel_stats.csv" % (TAG, cfg)))


def frame_march_rows(rows):
    """The frame-march rows, the one with the largest total duration first."""
    return sorted((r for r in rows if frame_march(r["Name"])), key=lambda r: -float(r["TotalDurationNs"]))


def instance(name):
    """"void march_pool_kernel<8, 1, 0, false, false, false>(MarchParams)" -> "march_pool_kernel<8, 1, 0, false, false, false>"."""
    name = name[len("void "):] if name.startswith("void ") else name
    return name.split(">")[0] + ">"
