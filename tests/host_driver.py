"""How a host twin is run under the sanitizers, and how the header is checked as plain C: the one
flag list, the objects of csrc/king_host.cc compiled once per process, the compile-and-run
recipe of the stand-alone drivers (tests/<feature>_host_driver.cc), and the C99 recipe.  A plain
module the tests import; a new feature adds a driver and one call of run_sanitized_driver.

The program is always a binary of its own with its own main(), run directly."""
import atexit
import re
import shutil
import subprocess
import tempfile
from functools import lru_cache
from pathlib import Path

from cuking_amd import build as b

TESTS = Path(__file__).resolve().parent

# king_host.cc as the library builds it (build.HIP_FLAGS: no contraction), plus the sanitizers;
# without -fno-sanitize-recover a UBSan finding prints and the program still exits 0.
SANITIZE_FLAGS = ["-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                  "-fno-sanitize-recover=undefined", f"-I{b.INCLUDE}", f"-I{b.CSRC}"]

# the last line of a driver's stdout: "0 failures", after a prefix that ends in no digit
NO_FAILURES = r"(?:.*\D)?0 failures"


@lru_cache(maxsize=None)
def sanitized_host_objects():
    """The files of build.HOST_ABI_SOURCES compiled with SANITIZE_FLAGS, once per process."""
    out = Path(tempfile.mkdtemp(prefix="cuking_host_objects_"))
    atexit.register(shutil.rmtree, out, ignore_errors=True)
    objects = []
    for name in b.HOST_ABI_SOURCES:
        objects.append(out / (Path(name).stem + ".o"))
        subprocess.run(["g++", *SANITIZE_FLAGS, "-c", str(b.CSRC / name), "-o",
                        str(objects[-1])], check=True)
    return tuple(objects)


def run_sanitized_driver(tmp_path, name, *, link_host=True, stdin=None, expect=None):
    """tests/<name>.cc built with SANITIZE_FLAGS, linked with the host objects, and run: exit
    status 0 and a last stdout line that matches `expect` as a whole, each on its own.  Returns
    the completed process."""
    exe = tmp_path / name
    objects = sanitized_host_objects() if link_host else ()
    subprocess.run(["g++", *SANITIZE_FLAGS, f"-I{TESTS}", str(TESTS / f"{name}.cc"),
                    *map(str, objects), "-o", str(exe)], check=True)
    p = subprocess.run([str(exe)], input=stdin, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    last = p.stdout.splitlines()[-1] if p.stdout.strip() else ""
    assert re.fullmatch(expect or NO_FAILURES, last), p.stdout + p.stderr
    return p


def compile_c99(tmp_path, source_text, run=False):
    """`source_text` as a C99 translation unit that includes cuking_amd.h: compiled with every
    warning an error, or, with run=True, also linked and run (exit status 0)."""
    src = tmp_path / "tu.c"
    src.write_text(source_text)
    out = tmp_path / ("tu" if run else "tu.o")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", f"-I{b.INCLUDE}",
                    *([] if run else ["-c"]), str(src), "-o", str(out)], check=True)
    if run:
        assert subprocess.run([str(out)]).returncode == 0
