"""div_row_weight4 (vlite-fast_amd/csrc/spectrum_div4.h), the spectrum step's division of a thread's four powers behind
one range test, against the IEEE division for every binary32: a stand-alone C++ program includes the header the
kernels include and runs all 2^32 bit patterns through member 0 of the group, while the other three members cycle
through the values that sit on the guard's edges.  Every one of the four outputs must be the bits of
x / 1.00000011920928955078125f (two NaNs count as equal).  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vlite-fast_amd", "csrc")

PROGRAM = r"""
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>
#include "spectrum_div4.h"

static inline uint32_t bits(float x) { uint32_t b; memcpy(&b, &x, 4); return b; }
static inline float val(uint32_t b) { float x; memcpy(&x, &b, 4); return x; }
static inline bool same(float got, float want)
{
    if (got != got || want != want) return got != got && want != want;
    return bits(got) == bits(want);
}
// 0, a denormal, the two values around the guard's lower edge, 1.0f, the largest finite float, +inf, a NaN
static const uint32_t EDGE[8] = {0u, 0x00000123u, 0x00800000u, 0x00800002u, 0x3f800000u, 0x7f7fffffu, 0x7f800000u, 0x7fc00000u};

int main()
{
    const float W = 1.00000011920928955078125f;
    if (bits(W) != 0x3f800001u) return 2;
    float edge_q[8];
    for (int e = 0; e < 8; ++e) edge_q[e] = val(EDGE[e]) / W;
    unsigned nthr = std::thread::hardware_concurrency();
    nthr = nthr < 1 ? 1 : nthr > 16 ? 16 : nthr;
    std::atomic<unsigned long long> bad(0), done(0);
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < nthr; ++t)
        pool.emplace_back([&, t]() {
            unsigned long long mybad = 0, mydone = 0;
            const uint64_t lo = ((uint64_t)1 << 32) * t / nthr, hi = ((uint64_t)1 << 32) * (t + 1) / nthr;
            for (uint64_t i = lo; i < hi; ++i) {
                const uint32_t b = (uint32_t)i;
                const unsigned e[4] = {0, b & 7, (b >> 3) & 7, (b >> 6) & 7};
                float x[4] = {val(b), val(EDGE[e[1]]), val(EDGE[e[2]]), val(EDGE[e[3]])};
                const float want[4] = {x[0] / W, edge_q[e[1]], edge_q[e[2]], edge_q[e[3]]};
                float p[4] = {x[0], x[1], x[2], x[3]};
                div_row_weight4(p, W, true);
                for (int q = 0; q < 4; ++q)
                    if (!same(p[q], want[q])) {
                        if (mybad++ < 4) fprintf(stderr, "group of %08x, member %d: %08x -> %08x, division gives %08x\n",
                                                 b, q, bits(x[q]), bits(p[q]), bits(want[q]));
                    }
                // the same entry point with another weight divides every value
                if ((b & 0xfffu) == 0x5a5u) {
                    const float w = 0.95999997854232788f;
                    float r[4] = {x[0], x[1], x[2], x[3]};
                    div_row_weight4(r, w, false);
                    for (int q = 0; q < 4; ++q)
                        if (!same(r[q], x[q] / w)) ++mybad;
                }
                ++mydone;
            }
            bad += mybad;
            done += mydone;
        });
    for (auto &th : pool) th.join();
    printf("%llu groups, %llu mismatches\n", (unsigned long long)done, (unsigned long long)bad);
    return bad ? 1 : 0;
}
"""


def test_four_wide_division_equals_ieee_division_for_every_float(tmp_path):
    src, exe = str(tmp_path / "div4.cpp"), str(tmp_path / "div4")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", "-I" + CSRC, "-o", exe, src], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0 and b"4294967296 groups, 0 mismatches" in r.stdout, (r.stdout, r.stderr[-2000:])


def test_kernels_use_the_checked_header():
    """both channelisers' spectrum steps go through the header (k_channelize_pfb.hip's unflagged rows have weight
    exactly 1 and need no division), and the header keeps the rule's constants"""
    src = open(os.path.join(CSRC, "k_channelize.hip")).read()
    assert '#include "spectrum_div4.h"' in src and "div_row_weight4(pw, wrow, kur_how == 1)" in src
    hdr = open(os.path.join(CSRC, "spectrum_div4.h")).read()
    assert "(b[q] & 0x7fffffu) - 1u" in hdr and "m1 >= 0x400001u ? 2u : 1u" in hdr and "0x00800002u" in hdr
