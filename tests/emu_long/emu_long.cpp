// emu_long.cpp -- TEST HARNESS ONLY: the long reads' passes of libgtx (gtx_hbm_passes.hip: gtx_align_long_kernel, then the
// exact pass gtx_align_exact_long(_wide)_kernel) run on the host through the sequential wavefront of tests/emu, behind the
// passes emu_align runs.  Like tests/emu it is never built into or loaded by libgtx.so.
#include "../emu/emu.cpp"
#include "../../graphtyper_amd/csrc/align_long.hpp"

extern "C"
{
  // emu_align, then -- as an align call of a context made with gtx_params::max_read_len > GTX_MAX_READ -- tier 1 and tier 2
  // over the reads of GTX_MAX_READ + 1 .. max_read_len bases.  tasks[5]: what gtx_ctx_long_pass_tasks reports.
  int emu_long_align(void * p, const uint8_t * nibble_rows, uint32_t nibble_stride, const gtx_read_meta * meta, uint32_t n_reads,
                     uint32_t * records, uint32_t rec_words, uint64_t * tasks)
  {
    using namespace gtx;
    int const rc = emu_align(p, nibble_rows, nibble_stride, meta, n_reads, records, rec_words);
    Emu & e = *static_cast<Emu *>(p);
    for (int k = 0; k < 5; ++k)
      tasks[k] = 0;
    uint32_t const max_len = e.params.max_read_len;
    if (rc != 0 || max_len <= GTX_MAX_READ || e.params.no_second_pass)
      return rc;
    uint32_t const seq_stride = (nibble_stride + PLANE_GROUP_BYTES - 1u) / PLANE_GROUP_BYTES * PLANE_GROUP_BYTES;
    std::vector<uint32_t> plane_rows(static_cast<size_t>(n_reads) * (seq_stride / 4) + 4);
    for (uint32_t r = 0; r < n_reads; ++r)
      planes_from_nibbles(nibble_rows + static_cast<uint64_t>(r) * nibble_stride, nibble_stride, plane_rows.data() + static_cast<size_t>(r) * (seq_stride / 4),
                          seq_stride / PLANE_GROUP_BYTES);
    uint8_t const * seq = reinterpret_cast<uint8_t const *>(plane_rows.data());
    GraphView const g = e.graph.view();
    IndexView const ix = e.index.view(static_cast<uint32_t>(e.params.max_index_labels), HALF_BUCKET_CAP);
    char const * fl = std::getenv("GTX_EMU_FILL");
    int const fill = fl ? std::atoi(fl) : 0xAB;
    bool has_wide_sites = false;
    uint32_t widest_site = 0;
    for (uint32_t n : e.graph.ref_nvar)
    {
      has_wide_sites = has_wide_sites || n > 64;
      widest_site = std::max(widest_site, n);
    }
    // (the slab emu_align made, cut as there)
    std::vector<uint8_t> & slab = e.exact_slab;
    uint64_t const exact_parts = std::min<uint64_t>(256u, std::max<uint64_t>(1u, (slab.size() >> 20) / (has_wide_sites ? 32u : 2u)));
    auto ws = std::make_unique<longr::AlignWorkspace>();
    std::vector<uint32_t> keys(2 * longr::AlignCfg::MAXPP, 0xABABABABu);
    std::vector<uint64_t> bits(longr::AlignCfg::MAXPP / 64 + 1, 0xABABABABABABABABull);
    auto claim = [&](uint32_t n) { return e.arena_claim(n); };
    // tier 2, the exact pass: a small part of the slab, a large part, all of it
    auto tier2 = [&](uint32_t read, uint32_t orient, uint32_t * rec, uint32_t len)
    {
      constexpr uint32_t TABLES = GTX_ST_LABEL_OVERFLOW | GTX_ST_PATH_OVERFLOW | GTX_ST_DFS_OVERFLOW;
      uint32_t last = TABLES;
      uint8_t const * row = seq + static_cast<uint64_t>(read) * seq_stride;
      uint32_t const cand_cap = exactl::exact_cand_cap(widest_site);
      for (uint32_t level = 0; level < EXACT_LAUNCHES && (last & TABLES); ++level)
      {
        ++tasks[1 + level];
        uint64_t const bytes = level == 0 ? ((slab.size() / exact_parts) & ~255ull) : level == 1 ? ((slab.size() / EXACT_LARGE_PARTS) & ~255ull) : slab.size();
        uint32_t const cap_v = level == 0 ? EXACT_PART_SITES : level == 1 ? EXACT_LARGE_SITES : has_wide_sites ? GTX_MAX_READ : GTX_MAX_READ_LONG;
        std::memset(slab.data(), fill, 65536);
        auto with_slab = [&](auto inst) // (a part that cannot hold one path: the task goes on as it came)
        {
          using I = decltype(inst);
          auto * xws = reinterpret_cast<typename I::Workspace *>(slab.data());
          if (I::template setup<WaveEmu>(xws, bytes, level == 0 ? std::min(cand_cap, EXACT_PART_CANDIDATES) : cand_cap, cap_v))
            last = I::template task<WaveEmu>(g, ix, *xws, row, len, orient == 1, rec, rec_words, e.arena.data(), e.arena.size(), claim);
        };
        if (has_wide_sites)
          with_slab(exactlw::Instance{});
        else
          with_slab(exactl::Instance{});
      }
      if (last & TABLES)
        ++tasks[4];
    };
    // tier 1 (gtx_align_long_kernel): each long read's slots by align_read's rules
    auto tier1 = [&](uint32_t read, uint32_t orient, uint32_t len)
    {
      ++tasks[0];
      uint32_t * rec = records + (2ull * read + orient) * rec_words;
      std::memset(static_cast<void *>(ws.get()), fill, sizeof(longr::AlignWorkspace));
      ws->pp_start = keys.data(); // (the kernel points them at LDS)
      ws->pp_end = keys.data() + longr::AlignCfg::MAXPP;
      ws->bits_pp = bits.data();
      uint8_t const * row = seq + static_cast<uint64_t>(read) * seq_stride;
      uint32_t const st = longr::align_one_arena<WaveEmu>(g, ix, *ws, row, len, orient == 1, rec, rec_words, e.arena.data(), e.arena.size(), claim);
      if (st)
        tier2(read, orient, rec, len);
    };
    bool const force_both = e.params.force_align_both_orientations != 0;
    for (uint32_t read = 0; read < n_reads; ++read)
    {
      gtx_read_meta const & m = meta[read];
      uint32_t const len = m.l_qseq;
      if (len <= GTX_MAX_READ || len > max_len)
        continue;
      tier1(read, 0, len);
      if (needs_reverse(m, force_both))
        tier1(read, 1, len);
      else if ((m.flag & GTX_FLAG_FORWARD_ONLY) == 0)
      {
        uint32_t * rec = records + (2ull * read + 1) * rec_words;
        rec[0] = 0;
        rec[1] = len << 16;
      }
    }
    return rc;
  }
}
