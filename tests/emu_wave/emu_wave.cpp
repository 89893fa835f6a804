// The sequential side of the wave policy (tests/wave_seq.hpp) held to the contract (graph_dev.hpp: the table): the probe's text
// (wave_probe.hpp), which gtx_wave_probe runs on the hardware wave, over gtx::WaveSeq, built with AddressSanitizer / UBSan.
//   emu_wave case.bin out.bin
// case.bin: uint32 n_sets; n_sets input sets of WP_IN_WORDS words.  out.bin: n_sets output sets of WP_OUT_WORDS words.
// Every set runs over heap blocks of exactly its sizes: a load or a store outside of the layout stops the program.
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "../wave_seq.hpp"
#include "wave_probe.hpp" // from the Makefile's CSRC

using namespace gtx;

int main(int argc, char ** argv)
{
  if (argc != 3)
  {
    std::fprintf(stderr, "usage: emu_wave case.bin out.bin\n");
    return 2;
  }
  std::FILE * f = std::fopen(argv[1], "rb");
  std::FILE * o = std::fopen(argv[2], "wb");
  uint32_t n_sets = 0;
  if (!f || !o || std::fread(&n_sets, 4, 1, f) != 1)
    return 2;
  for (uint32_t s = 0; s < n_sets; ++s)
  {
    std::unique_ptr<uint32_t[]> in(new uint32_t[WP_IN_WORDS]), out(new uint32_t[WP_OUT_WORDS]);
    if (std::fread(in.get(), 4, WP_IN_WORDS, f) != WP_IN_WORDS)
      return 2;
    wave_probe_start(in.get(), out.get());
    wave_probe<WaveSeq>(in.get(), out.get());
    if (std::fwrite(out.get(), 4, WP_OUT_WORDS, o) != WP_OUT_WORDS)
      return 2;
  }
  std::fclose(f);
  return std::fclose(o) == 0 ? 0 : 2;
}
