"""Both feature lists of a position from one board walk (fishnet_amd/csrc/plan_lists.h) on the host.

tests/plan_lists_host.cpp calls the host build of build_list_pair, the builder plan_scatter_kernel
runs per lane, under AddressSanitizer + UndefinedBehaviorSanitizer and checks the list contract
against a naive per-square reference of its own: for each perspective and each item parity, the
entries' multiset, the two parity runs and their lengths, the padding, and that nothing outside
the staging row and the two lists is written.  Boards: two bare kings, 32 pieces, kings on files
a-d / e-h and in the same / different half boards in every combination, all other pieces on even
or on odd files only, all pieces in one half board, every pair of king squares, and 6,000 random
placements of 2 to 32 pieces.  CPU only; the program is run directly, nothing is preloaded."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.mark.parametrize("opt", ["-O1", "-O2"])
def test_list_pair_contract_under_asan_ubsan(tmp_path, opt):
    exe = tmp_path / "plan_lists_host"
    subprocess.run(["g++", "-std=c++17", opt, "-Wall", "-Werror", *SAN, "-I", os.path.join(ROOT, "fishnet_amd/csrc"),
                    os.path.join(ROOT, "tests/plan_lists_host.cpp"), "-o", str(exe)], check=True)
    # verify_asan_link_order=0: the environment may preload a library ahead of the ASan runtime
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "plan lists ok" in r.stdout
    assert int(r.stdout.split()[-2]) > 10000
