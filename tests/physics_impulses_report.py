"""The compiler's resource report of the batched object physics with scripted accelerations' translation unit
(python_raytracer_amd/csrc/vrt_physics_impulses.hip), by the recipe of tests/kernel_report.py pointed at that file, and the
saved copy tests/test_physics_impulses_host.py holds it to.

    python tests/physics_impulses_report.py --write    regenerates profiles/physics_impulses_kernel_resource_usage.txt"""
import os
import subprocess
import sys
import tempfile

import kernel_report

SRC = os.path.join(kernel_report.ROOT, "python_raytracer_amd", "csrc", "vrt_physics_impulses.hip")
SAVED = os.path.join(kernel_report.ROOT, "profiles", "physics_impulses_kernel_resource_usage.txt")


def compile_report():
    """The compiler's remarks (its stderr) for the source in the tree: one device-only compile for gfx950, no GPU needed."""
    with tempfile.TemporaryDirectory() as tmp:
        p = subprocess.run([kernel_report.HIPCC, "-O3", "--offload-arch=gfx950", "-ffp-contract=off", "-std=c++17", "--cuda-device-only",
                            "-c", "-Rpass-analysis=kernel-resource-usage", SRC, "-o", os.path.join(tmp, "vrt_physics_impulses.o")],
                           capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stderr


def saved():
    with open(SAVED) as f:
        return kernel_report.parse(f.read())


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit(__doc__)
    text = kernel_report.saved_text(compile_report())
    with open(SAVED, "w") as f:
        f.write(text)
    print("%s: %d functions" % (os.path.relpath(SAVED, kernel_report.ROOT), len(kernel_report.parse(text))))
