"""The launch dispatcher of every entry that walks the hash grid (csrc/kernels/field_dispatch.hiph) on
its own: a stand-alone host program includes the header -- it needs no HIP -- and checks, under the
address and undefined-behaviour sanitizers, that each (F, T) reaches the callback exactly once with
that F and with POW2 == (T is a power of two), that each (L, F) of the one-pass render family reaches
it exactly once with C = L * F, and that the pair beyond the level cap reaches nothing.  A
power-of-two table routed to the general-modulus kernel would compute the same values, only slower:
this is where that mistake would show."""
import importlib
import os
import subprocess

build = importlib.import_module("f2-nerf_amd._build")

PROGRAM = r"""
#include "field_dispatch.hiph"

#include <cstdio>
#include <cstdlib>

#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);        \
      std::exit(1);                                                  \
    }                                                                \
  } while (0)

static bool pow2_by_counting(uint32_t v)
{
  int ones = 0;
  for (int b = 0; b < 32; b++) ones += (v >> b) & 1u;
  return ones == 1;
}

int main()
{
  const int Fs[] = {1, 2, 4, 8};
  const uint32_t Ts[] = {1u, 2u, 3u, 1000u, 4096u, 5000u, 1u << 19, (1u << 19) + 1u, 0x80000000u,
                         0xffffffffu};
  int checked = 0;
  for (int F : Fs)
    for (uint32_t T : Ts) {
      CHECK(f2n_is_pow2(T) == pow2_by_counting(T));
      int calls = 0, got_f = 0;
      bool got_p2 = false;
      f2n_dispatch_field(F, T, [&](auto ff, auto p2) {
        constexpr int FF = decltype(ff)::value;    // (compile-time constants: usable as
        constexpr bool P2 = decltype(p2)::value;   //  template arguments of a kernel)
        calls++;
        got_f = FF;
        got_p2 = P2;
      });
      CHECK(calls == 1);
      CHECK(got_f == F);
      CHECK(got_p2 == pow2_by_counting(T));
      checked++;
    }
  CHECK(checked == 40);
  CHECK(!f2n_is_pow2(0u));

  int pairs = 0;
  const int Cs[] = {8, 16, 32, 64};
  for (int C : Cs)
    for (int F : Fs) {
      const int L = C / F;
      if (L > F2N_MAX_LEVELS) continue;
      for (uint32_t T : Ts) {
        int calls = 0, got_c = 0, got_f = 0;
        bool got_p2 = false;
        f2n_dispatch_width_field(L, F, T, [&](auto cc, auto ff, auto p2) {
          constexpr int CC = decltype(cc)::value;
          constexpr int FF = decltype(ff)::value;
          constexpr bool P2 = decltype(p2)::value;
          static_assert(CC / FF <= F2N_MAX_LEVELS, "a pair beyond the level cap was instantiated");
          calls++;
          got_c = CC;
          got_f = FF;
          got_p2 = P2;
        });
        CHECK(calls == 1);
        CHECK(got_c == L * F && got_f == F);
        CHECK(got_p2 == pow2_by_counting(T));
      }
      pairs++;
    }
  CHECK(pairs == 15);  // x 2 for POW2: the 30 instantiations of each kernel of the family

  for (uint32_t T : Ts) {
    int calls = 0;
    f2n_dispatch_width_field(64, 1, T, [&](auto, auto, auto) { calls++; });
    CHECK(calls == 0);
  }
  std::puts("field dispatch ok");
  return 0;
}
"""


def test_dispatcher_stand_alone_under_sanitizers(tmp_path):
    src, exe = tmp_path / "field_dispatch_main.cpp", tmp_path / "field_dispatch_main"
    src.write_text(PROGRAM)
    cxx = os.environ.get("CXX", "g++")
    # (the sanitizer runtimes are linked in: the program carries its own, whatever else is loaded)
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", build.INCLUDE_DIR,
           "-I", build.KERNEL_DIR, "-x", "c++", str(src), "-o", str(exe)]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-4000:]
    res = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-4000:]
    assert "field dispatch ok" in res.stdout
