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
    // (the slab emu_align made, cut as there: CallScratch's constants)
    constexpr uint32_t EXACT_PART_SITES = 24, EXACT_PART_CANDIDATES = 8256, EXACT_LARGE_PARTS = 32, EXACT_LARGE_SITES = 64;
    std::vector<uint8_t> & slab = e.exact_slab;
    uint64_t const exact_parts = std::min<uint64_t>(256u, std::max<uint64_t>(1u, (slab.size() >> 20) / (has_wide_sites ? 32u : 2u)));
    auto ws = std::make_unique<longr::AlignWorkspace>();
    std::vector<uint32_t> keys(2 * longr::AlignCfg::MAXPP, 0xABABABABu);
    std::vector<uint64_t> bits(longr::AlignCfg::MAXPP / 64 + 1, 0xABABABABABABABABull);
    // one task through a pass: the body of GTX_HBM_PASS_BODY (gtx_hbm_passes.hip); returns the pass' raw status
    auto pass = [&](auto && align, auto && size_of, auto && write_body, uint32_t * rec, uint32_t len) -> uint32_t
    {
      uint32_t np = 0, longest = 0, ext = 0;
      uint32_t const raw = align(np, longest);
      uint32_t status = raw & ~GTX_ST_WIDE_ALLELE;
      uint32_t * body = rec + 2;
      uint64_t off = 0;
      if (status)
        np = 0;
      else
      {
        uint32_t const size = size_of(np);
        if (size > rec_words)
        {
          off = e.arena_used;
          if (off + (size - 2) > e.arena.size())
          {
            status = GTX_ST_RECORD_OVERFLOW;
            np = 0;
          }
          else
          {
            e.arena_used += size - 2;
            body = e.arena.data() + off;
            ext = GTX_ST_EXTERNAL;
          }
        }
      }
      uint32_t const has_var = write_body(np, body);
      rec[0] = np | ((status | ext) << 16);
      rec[1] = (np == 0 ? 0 : longest) | (len << 16) | (np == 0 ? 0u : has_var);
      if (ext)
        rec[2] = static_cast<uint32_t>(off);
      return raw;
    };
    // tier 2, the exact pass: a small part of the slab, a large part, all of it
    auto tier2 = [&](uint32_t read, uint32_t orient, uint32_t * rec, uint32_t len)
    {
      constexpr uint32_t TABLES = GTX_ST_LABEL_OVERFLOW | GTX_ST_PATH_OVERFLOW | GTX_ST_DFS_OVERFLOW;
      uint32_t last = TABLES;
      uint8_t const * row = seq + static_cast<uint64_t>(read) * seq_stride;
      for (uint32_t level = 0; level < 3 && (last & TABLES); ++level)
      {
        ++tasks[1 + level];
        uint64_t const bytes = level == 0 ? ((slab.size() / exact_parts) & ~255ull) : level == 1 ? ((slab.size() / EXACT_LARGE_PARTS) & ~255ull) : slab.size();
        uint32_t const cap_v = level == 0 ? EXACT_PART_SITES : level == 1 ? EXACT_LARGE_SITES : has_wide_sites ? GTX_MAX_READ : GTX_MAX_READ_LONG;
        std::memset(slab.data(), fill, 65536);
        if (has_wide_sites)
        {
          auto * xws = reinterpret_cast<exactlw::AlignWorkspace *>(slab.data());
          if (!exactlw::exact_setup<WaveEmu>(xws, bytes, level == 0 ? std::min(exactlw::exact_cand_cap(widest_site), EXACT_PART_CANDIDATES) : exactlw::exact_cand_cap(widest_site), cap_v))
            continue;
          last = pass([&](uint32_t & np, uint32_t & longest) { return exactlw::align_paths<WaveEmu>(g, ix, *xws, row, len, orient == 1, np, longest); },
                      [&](uint32_t np) { return exactlw::record_size<WaveEmu>(exactlw::Here{}, *xws, np); },
                      [&](uint32_t np, uint32_t * body) { return exactlw::write_record_body<WaveEmu>(exactlw::Here{}, *xws, np, body); }, rec, len);
        }
        else
        {
          auto * xws = reinterpret_cast<exactl::AlignWorkspace *>(slab.data());
          if (!exactl::exact_setup<WaveEmu>(xws, bytes, level == 0 ? std::min(exactl::exact_cand_cap(widest_site), EXACT_PART_CANDIDATES) : exactl::exact_cand_cap(widest_site), cap_v))
            continue;
          last = pass([&](uint32_t & np, uint32_t & longest) { return exactl::align_paths<WaveEmu>(g, ix, *xws, row, len, orient == 1, np, longest); },
                      [&](uint32_t np) { return exactl::record_size<WaveEmu>(exactl::Here{}, *xws, np); },
                      [&](uint32_t np, uint32_t * body) { return exactl::write_record_body<WaveEmu>(exactl::Here{}, *xws, np, body); }, rec, len);
        }
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
      uint32_t const st = pass([&](uint32_t & np, uint32_t & longest) { return longr::align_paths<WaveEmu>(g, ix, *ws, row, len, orient == 1, np, longest); },
                               [&](uint32_t np) { return longr::record_size<WaveEmu>(longr::Here{}, *ws, np); },
                               [&](uint32_t np, uint32_t * body) { return longr::write_record_body<WaveEmu>(longr::Here{}, *ws, np, body); }, rec, len);
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
