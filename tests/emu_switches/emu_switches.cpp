// The readers of the library's environment switches (gtx_switches.hpp) as a program of their own, built with AddressSanitizer / UBSan.
//   emu_switches case.txt out.txt
// case.txt, line by line: `NAME=VALUE` sets a variable (VALUE may be empty), `-NAME` unsets it, `?` calls every reader and writes one
// line of `reader=value` words to out.txt.  tests/test_switches.py compares the lines with a table written there.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "graph_dev.hpp"    // HALF_BUCKET_CAP
#include "gtx_switches.hpp" // from the Makefile's CSRC

using namespace gtx;

static void report(std::FILE * o)
{
  sw::AlignSwitches const a = sw::align_switches();
  // (wide / dense where the graph would choose lean and where it would choose the other build: a forced build shows in both)
  std::fprintf(o, "force=%u four=%d hinted=%d decline_all=%d wide=%d%d hint_dense=%d%d hint_less=%u", a.force, a.four, a.hinted, a.decline_all, a.wide(false),
               a.wide(true), a.hint_dense(false), a.hint_dense(true), a.hint_less);
  std::fprintf(o, " hint_more=%d nb_known=%d index_runs=%d build_stream=%d big_grid_adaptive=%d bgzf_crc=%d timing=%d", sw::hint_more(), sw::nb_known(),
               sw::index_runs(), sw::build_stream(), sw::big_grid_adaptive(), sw::bgzf_crc(), sw::timing());
  std::fprintf(o, " host_threads=%u half_bucket_cap=%u hint_windows=%llu device_cache_mb=%llu time_every=%u", sw::host_threads(), sw::half_bucket_cap(HALF_BUCKET_CAP),
               static_cast<unsigned long long>(sw::hint_windows()), static_cast<unsigned long long>(sw::device_cache_mb()), sw::time_every());
  std::fprintf(o, " bgzf_threads=%u bgzf_linger_us=%d bgzf_device_ring=%u bgzf_device=%d inflate_zlib=%d", sw::bgzf_threads(16), sw::bgzf_linger_us(300),
               sw::bgzf_device_ring(32), sw::bgzf_device(), sw::inflate_zlib());
  std::fprintf(o, " exact_pass_mb=%llu exact_parts=%u\n", static_cast<unsigned long long>(sw::exact_pass_mb()), sw::exact_parts());
}

int main(int argc, char ** argv)
{
  if (argc != 3)
  {
    std::fprintf(stderr, "usage: emu_switches case.txt out.txt\n");
    return 2;
  }
  std::FILE * f = std::fopen(argv[1], "r");
  std::FILE * o = std::fopen(argv[2], "w");
  if (!f || !o)
    return 2;
  char buf[512];
  while (std::fgets(buf, sizeof buf, f))
  {
    std::string line(buf);
    while (!line.empty() && (line.back() == '\n' || line.back() == '\r'))
      line.pop_back();
    size_t const eq = line.find('=');
    if (line == "?")
      report(o);
    else if (!line.empty() && line[0] == '-')
      unsetenv(line.c_str() + 1);
    else if (eq != std::string::npos && eq > 0)
      setenv(line.substr(0, eq).c_str(), line.c_str() + eq + 1, 1);
    else
      return 2;
  }
  std::fclose(f);
  return std::fclose(o) == 0 ? 0 : 2;
}
