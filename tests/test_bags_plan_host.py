"""csrc/bags_plan.hpp alone on the host, plainly and as a stand-alone program under the address and undefined-behaviour
sanitizers: the domain of dlrm_bags_interact_fwd on both sides of each limit, the column block at NB = 3 / 4 and below
a block, the two tiles within 64 KB over the whole domain; and the entry point's argument checks."""
import os
import shutil
import subprocess

import pytest

CASES = [  # dtype d T lookups tabs16 x_address x_ld ys_address ys_ld -> in the domain
    ((0, 256, 64, 10, 1, 4096, 256, 0, 0), 1), ((1, 256, 64, 10, 1, 4096, 256, 8192, 16640), 1),
    ((0, 16, 95, 2, 1, 4096, 16, 0, 0), 1), ((0, 16, 96, 2, 1, 4096, 16, 0, 0), 0), ((0, 16, 0, 2, 1, 4096, 16, 0, 0), 0),
    ((0, 16, 7, 1, 1, 4096, 16, 0, 0), 1), ((0, 16, 7, 0, 1, 4096, 16, 0, 0), 0),
    ((0, 12, 7, 2, 1, 4096, 12, 0, 0), 1), ((1, 12, 7, 2, 1, 4096, 16, 0, 0), 0), ((0, 14, 7, 2, 1, 4096, 16, 0, 0), 0),
    ((0, 16, 7, 2, 0, 4096, 16, 0, 0), 0), ((0, 16, 7, 2, 1, 4112, 16, 0, 0), 1), ((0, 16, 7, 2, 1, 4100, 16, 0, 0), 0),
    ((0, 16, 7, 2, 1, 4096, 18, 0, 0), 0), ((1, 16, 7, 2, 1, 4096, 20, 0, 0), 0), ((1, 16, 7, 2, 1, 4096, 24, 0, 0), 1),
    ((0, 16, 7, 2, 1, 4096, 16, 8192, 128), 1), ((0, 16, 7, 2, 1, 4096, 16, 8196, 128), 0),
    ((0, 16, 7, 2, 1, 4096, 16, 8192, 130), 0), ((1, 16, 7, 2, 1, 4096, 16, 8192, 132), 0),
    ((0, 256, 47, 2, 1, 4096, 256, 0, 0), 1), ((0, 256, 48, 2, 1, 4096, 256, 0, 0), 1),
    ((1, 136, 32, 9, 1, 4096, 136, 0, 0), 1), ((0, 136, 32, 9, 1, 4096, 136, 0, 0), 1),
]

def _want(dtype, d, T):
    nb = (T + 16) // 16
    cb = min(512 if nb <= 3 else 256, (d * (4, 2)[dtype] + 63) // 64 * 64)
    return cb, 2 * 16 * nb * (cb + 16)

@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "asan-ubsan"])
def test_plan_header_alone_on_the_host(tmp_path, flags):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "plan")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", *flags, "-o", exe,
                    os.path.join(os.path.dirname(os.path.abspath(__file__)), "bags_plan_print.cpp")], check=True)
    text = "".join(" ".join(str(v) for v in c) + "\n" for c, _ in CASES)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    got = [tuple(int(v) for v in line.split()) for line in out[:len(CASES)]]
    assert got == [(ok, *_want(*c[:3])) for c, ok in CASES]
    by = {c[:3]: g for (c, _), g in zip(CASES, got)}
    assert by[(0, 256, 47)][1] == 512 and by[(0, 256, 48)][1] == 256  # NB = 3 / 4
    assert by[(0, 12, 7)][1] == 64 and by[(1, 136, 32)][1] == 320      # a row below a block: whole column steps
    assert out[len(CASES)].split() == ["max", "52224", "50688", "52224"]  # <= 65536, at NB = 6 and NB = 3

def test_entry_point_checks_its_arguments_without_a_device(pkg):
    lib = pkg._lib.load()
    assert lib.dlrm_bags_interact_fwd(None, None, None, 0, 0, 0, 1, 1, None, 16, None, 0, None, 17, 0) == pkg._lib.E_ARG
    assert lib.dlrm_abi_version() == 9
