"""csrc/kept_inputs.h, the one record of the inputs that a kept result was derived from (the light shafts' verdicts per frame
context, the prepared polygons per pass): tests/kept_inputs_check.cpp, a program with its own main, is compiled against the
header alone with the host compiler of csrc/Makefile and run.  It asserts: a first image equals nothing; an identical one
equals in its prefix and in every record; one changed record differs alone; an image of another size, and any image after
a forget, equals nothing; growing keeps the kept bytes; an image without records works; a failed allocation forgets."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vulkan_renderer_amd", "csrc")


def test_kept_inputs_stand_alone(tmp_path):
    # (what $(CC) is once make has read the Makefile and the environment)
    compiler = subprocess.run(["make", "-s", "-C", CSRC, "--no-print-directory", "--eval", "print-host-compiler: ; @echo $(CC)", "print-host-compiler"],
                              capture_output=True, text=True, timeout=60, check=True).stdout.split()
    assert compiler, "csrc/Makefile names no host compiler"
    program = str(tmp_path / "kept_inputs_check")
    built = subprocess.run(compiler + ["-x", "c++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "kept_inputs_check.cpp"), "-o", program],
                           capture_output=True, text=True, timeout=120)
    assert built.returncode == 0, built.stdout + built.stderr
    done = subprocess.run([program], capture_output=True, text=True, timeout=60)
    assert done.returncode == 0 and done.stdout.strip() == "kept_inputs ok", done.stdout + done.stderr
