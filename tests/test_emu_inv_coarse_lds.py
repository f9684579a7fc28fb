"""The residency assumption of the inverse coarse group (pypwt_amd/csrc/launch_dwt2_inv_coarse.hip): on the 2048^2 plane of the
headline plan the 64 x 32 / 512 tile of db4 is ONE round of 512 workgroups only while two of them fit a CU's 160 KiB of LDS -- its
79.5 KiB.  A tiny probe compiled here with g++ (-DPDWT_CPU_EMU, as tests/cpu_emu) prints InvCoarse3Geom<8,64,32>::LDS_FLOATS, so
that a change to the staged regions cannot grow past that silently.  CPU only."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "pypwt_amd", "csrc", "dwt2_inv_coarse_kernels.hpp")

PROBE = """#define PDWT_CPU_EMU 1
#include <cstdio>
#include "%s"
int main() {
    std::printf("%%d\\n", pdwt::InvCoarse3Geom<8, 64, 32>::LDS_FLOATS);
    return 0;
}
"""


def test_the_headline_tile_of_the_coarse_group_stays_within_its_lds(tmp_path):
    src, exe = str(tmp_path / "probe.cpp"), str(tmp_path / "probe")
    with open(src, "w") as f:
        f.write(PROBE % HEADER)
    subprocess.check_call(["g++", "-O0", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", "-o", exe, src])
    floats = int(subprocess.check_output([exe]).decode())
    print("InvCoarse3Geom<8,64,32>::LDS_FLOATS = %d (%.2f KiB)" % (floats, floats * 4 / 1024.0))
    assert floats * 4 <= 79.5 * 1024, floats
    assert 2 * floats * 4 <= 160 * 1024, "two workgroups per CU"
