"""The compiler's resource report of the shipped HIP source, compiled once, and the saved copy every figure is pinned by.

    report()  {mangled name: {figure: int}} of every device function, in the order the compiler emits them: one device-only
              compile for gfx950 with -Rpass-analysis=kernel-resource-usage (no GPU needed), once per process
    saved()   the same, read from profiles/kernel_resource_usage.txt

    python tests/kernel_report.py --write    regenerates profiles/kernel_resource_usage.txt: a kernel change that moves a figure
                                             on purpose commits the new file with it

The saved file holds, per function and in emission order, the `Function Name:` line and the eight figures as the compiler
prints them, without the `<file>:<line>:<col>: remark:` in front and the flag's name behind, so that a moved line changes
nothing in it."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "python_raytracer_amd", "csrc", "vrt_kernels.hip")
SAVED = os.path.join(ROOT, "profiles", "kernel_resource_usage.txt")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FIGURES = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill",
           "LDS Size [bytes/block]")
_report = None


def parse(text):
    """{name: {figure: int}} of a report: the compiler's remarks or the saved file's lines."""
    blocks = {}
    for b in re.split(r"(?=Function Name: )", text):
        m = re.match(r"Function Name: (\S+)", b)
        if m:
            assert m.group(1) not in blocks, "reported twice: " + m.group(1)
            blocks[m.group(1)] = {k: int(v) for k, v in re.findall(r"\n(?:.*remark:)?\s+([A-Za-z \[\]/]+): (\d+)", b)}
    return blocks


def compile_report():
    """The compiler's remarks (its stderr) for the source in the tree."""
    with tempfile.TemporaryDirectory() as tmp:
        p = subprocess.run([HIPCC, "-O3", "--offload-arch=gfx950", "-ffp-contract=off", "-std=c++17", "--cuda-device-only", "-c",
                            "-Rpass-analysis=kernel-resource-usage", SRC, "-o", os.path.join(tmp, "vrt.o")],
                           capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stderr


def report():
    global _report
    if _report is None:
        if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
            import pytest
            pytest.skip("no hipcc")
        _report = parse(compile_report())
    return _report


def saved():
    with open(SAVED) as f:
        return parse(f.read())


def saved_text(remarks):
    """The saved file's text for the compiler's remarks."""
    lines = []
    for line in remarks.splitlines():
        m = re.match(r".*remark: (Function Name: \S+|\s+(%s): \d+) \[" % "|".join(re.escape(f) for f in FIGURES), line)
        if m:
            lines.append(m.group(1))
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit(__doc__)
    text = saved_text(compile_report())
    with open(SAVED, "w") as f:
        f.write(text)
    print("%s: %d functions" % (os.path.relpath(SAVED, ROOT), len(parse(text))))
