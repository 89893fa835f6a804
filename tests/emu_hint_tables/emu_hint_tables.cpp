// The seven tables of the position-hinted pass (gtx_ctx_hint_table 0..6) as a context without a device builds them: flatten_graph and
// build_index of graphtyper_amd/csrc/gtx_host.cpp, which run the text of index_build.hpp -- both compiled into this program as they
// stand, with AddressSanitizer / UBSan.
//   emu_hint_tables case.bin out.bin
// case.bin: uint32 is_sv_graph, n_ref, n_var, dna_len, n_event_values; the node tables as gtx_graph_view names them, uint32 each -- ref_order, ref_len,
//   ref_dna_off, ref_nvar, ref_first_var [n_ref], var_order, var_len, var_dna_off, var_out_ref [n_var] --; the graph's characters; with
//   n_event_values != 0 the alleles' events: uint32 event_off [2 n_var + 1], int64 event_val [n_event_values].
//   (The graph is the one gtx_graph_build made of the case's reference and records: tests/hint_tables_cases.py; the constructor has its
//   own tests and needs the device runtime's headers, this program does not.)
// out.bin: for each of the tables 0..6, uint64 number of words and the words.
// Every input is a heap block of exactly its size: a load outside of one stops the program.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "gtx_host.cpp" // from the Makefile's CSRC, and with it that directory's index_build.hpp

namespace
{
bool read_exact(std::FILE * f, void * p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }
bool write_exact(std::FILE * f, void const * p, size_t n) { return n == 0 || std::fwrite(p, 1, n, f) == n; }

std::unique_ptr<uint32_t[]> block(std::FILE * f, size_t n, bool & ok)
{
  std::unique_ptr<uint32_t[]> p(new uint32_t[n]);
  ok = ok && read_exact(f, p.get(), n * sizeof(uint32_t));
  return p;
}

bool put(std::FILE * f, void const * words, uint64_t n_words)
{
  return write_exact(f, &n_words, sizeof n_words) && write_exact(f, words, n_words * sizeof(uint32_t));
}
} // namespace

int main(int argc, char ** argv)
{
  if (argc != 3)
  {
    std::fprintf(stderr, "usage: %s case.bin out.bin\n", argv[0]);
    return 2;
  }
  std::FILE * f = std::fopen(argv[1], "rb");
  uint32_t head[5];
  if (!f || !read_exact(f, head, sizeof head))
  {
    std::fprintf(stderr, "cannot read %s\n", argv[1]);
    return 2;
  }
  uint32_t const is_sv = head[0], R = head[1], V = head[2], n_dna = head[3], n_events = head[4];
  bool ok = true;
  auto ref_order = block(f, R, ok), ref_len = block(f, R, ok), ref_dna = block(f, R, ok), ref_nvar = block(f, R, ok), ref_first_var = block(f, R, ok);
  auto var_order = block(f, V, ok), var_len = block(f, V, ok), var_dna = block(f, V, ok), var_out_ref = block(f, V, ok);
  std::unique_ptr<char[]> dna(new char[n_dna]);
  ok = ok && read_exact(f, dna.get(), n_dna);
  auto event_off = block(f, n_events ? 2 * static_cast<size_t>(V) + 1 : 0, ok);
  std::unique_ptr<int64_t[]> event_val(new int64_t[n_events]);
  ok = ok && read_exact(f, event_val.get(), n_events * sizeof(int64_t));
  std::fclose(f);
  if (!ok)
  {
    std::fprintf(stderr, "%s is too short\n", argv[1]);
    return 2;
  }
  gtx_graph_view view{};
  view.n_ref = R;
  view.n_var = V;
  view.ref_order = ref_order.get();
  view.ref_len = ref_len.get();
  view.ref_dna_off = ref_dna.get();
  view.ref_nvar = ref_nvar.get();
  view.ref_first_var = ref_first_var.get();
  view.var_order = var_order.get();
  view.var_len = var_len.get();
  view.var_dna_off = var_dna.get();
  view.var_out_ref = var_out_ref.get();
  view.dna = dna.get();
  view.dna_len = n_dna;
  if (n_events)
  {
    view.event_off = event_off.get();
    view.event_val = event_val.get();
  }
  gtx_params par{};
  par.max_index_labels = 75;
  par.is_sv_graph = static_cast<int32_t>(is_sv);
  par.sam_flag_filter = 3840;
  gtx::HostGraph graph;
  std::string const msg = gtx::flatten_graph(view, par, graph);
  if (!msg.empty())
  {
    std::fprintf(stderr, "flatten_graph: %s\n", msg.c_str());
    return 2;
  }
  gtx::HostIndex index;
  gtx::build_index(graph, index);
  static_assert(sizeof(gtx::uint2_t) == 8 && sizeof(gtx::HintWindow) == 32, "the tables' words");
  std::FILE * o = std::fopen(argv[2], "wb");
  // (what gtx_ctx_hint_table hands out: the tables' whole lengths, and no site_win without windows)
  bool const wrote = o && put(o, index.pos_flags.data(), 2 * index.pos_flags.size()) && put(o, index.refp.data(), index.refp.size()) &&
                     put(o, index.tail_info.data(), 2 * index.tail_info.size()) && put(o, index.filt[0].data(), index.filt[0].size()) &&
                     put(o, index.filt[1].data(), index.filt[1].size()) && put(o, index.win.data(), 8 * index.win.size()) &&
                     put(o, index.site_win.data(), index.win.empty() ? 0 : index.site_win.size());
  if (!wrote || std::fclose(o) != 0)
  {
    std::fprintf(stderr, "cannot write %s\n", argv[2]);
    return 2;
  }
  return 0;
}
