// gtx_inflate_dev.hpp -- raw DEFLATE (RFC 1951) decoder for BGZF members, kernel source: one wavefront inflates one member.
//
// Written against the wave policy of graph_dev.hpp (wave-uniform state + lane lambdas): gtx_inflate_dev.hip instantiates it
// with the hardware wave, tests/emu_inflate with a sequential one under AddressSanitizer.  The host decoder (gtx_inflate.hpp)
// may leave a member to zlib when its second-level tables outgrow their room; there is no zlib here, so every complete code
// of RFC 1951 is decoded in fixed memory:
//   * per alphabet the canonical form count[len] / sorted[] (symbols by length, then value) in LDS, which alone decodes any
//     code of up to 15 bits by the walk over the lengths (first code of a length, number of codes of it);
//   * in front of it a first-level table (10 bits literal/length, 8 bits distance, 16-bit entries: symbol << 4 | length) that
//     the 64 lanes fill by running that walk for the table's indices; 0 = not a code of that few bits -> the walk.
//   4 096 bytes of LDS per wavefront, so LDS never bounds the occupancy (32 wavefronts of a CU take 128 of its 160 KB).
// The walk over the codes is wave-uniform (every lane holds the same bit buffer; table reads are broadcasts).  What it decodes
// goes to a batch of 64 tokens in LDS; a full batch is written by the wavefront: the literals one per lane, then the matches
// in order, each copied by all lanes (byte i from src[i % dist] when the distance is shorter than the length).  The output
// is in global memory and a match reads what earlier tokens wrote, so stores are fenced before such a read -- once per batch
// in front of the matches, and again only where a match reads from a match of the same batch.
// Bounds: no load outside [in, in + in_len), no store outside [out, out + out_len), a match that reaches in front of the output is
// refused, and every loop consumes input bits or produces output bytes (`overrun`: more bits taken than the stream has).
#pragma once
#include <cstdint>

#include "graph_dev.hpp"

namespace gtx
{
// status of a member (include/gtx.h: GTX_INFLATE_*)
constexpr uint32_t INFL_OK = 0, INFL_BAD_STREAM = 1, INFL_SHORT = 2, INFL_LONG = 3, INFL_CRC = 4, INFL_BAD_MEMBER = 5;
constexpr uint32_t INFL_MAX_OUT = 65536;
constexpr uint32_t INFL_LIT_BITS = 10, INFL_DIST_BITS = 8, INFL_TOKENS = 64;
constexpr uint32_t INFL_TOK_MATCH = 0x80000000u;

struct InflateMember // gtx_inflate_member
{
  uint64_t in_off, out_off;
  uint32_t in_len, out_len, crc32, reserved;
};

struct InflateWs
{
  uint16_t lit_tab[1u << INFL_LIT_BITS];
  uint16_t dist_tab[1u << INFL_DIST_BITS]; // (the code-length code's 7-bit table while a block's header is read)
  uint16_t lit_sorted[288], dist_sorted[32];
  uint16_t lit_count[16], dist_count[16];
  uint32_t tok_pos[INFL_TOKENS];   // offset in the member's output | INFL_TOK_MATCH
  uint32_t tok_val[INFL_TOKENS];   // the literal, or length << 16 | distance - 1
  uint8_t lens[288 + 32];
};
static_assert(sizeof(InflateWs) == 4096, "the LDS a wavefront takes, as the documents state it");

namespace inflate_dev
{
GTX_DEV uint32_t len_base(uint32_t s) // symbol 257 + s
{
  return s < 8 ? 3 + s : s == 28 ? 258 : 3 + ((4 + (s & 3u)) << ((s >> 2) - 1));
}
GTX_DEV uint32_t len_extra(uint32_t s) { return s < 8 || s == 28 ? 0 : (s >> 2) - 1; }
GTX_DEV uint32_t dist_base(uint32_t s) { return s < 4 ? 1 + s : 1 + ((2 + (s & 1u)) << ((s >> 1) - 1)); }
GTX_DEV uint32_t dist_extra(uint32_t s) { return s < 4 ? 0 : (s >> 1) - 1; }

// the member's input as a bit stream (wave-uniform): gtx_inflate.hpp's reader, with the stream's last bytes loaded one by one
struct Bits
{
  uint8_t const * in;
  int32_t in_len, ip;
  uint64_t buf;
  uint32_t cnt;
};

template <class W>
GTX_DEV void refill(Bits & b)
{
  if (b.ip < b.in_len)
  {
    uint64_t w = 0;
    if (b.ip + 8 <= b.in_len)
    {
      uint8_t const * p = b.in + b.ip;
      uint64_t v;
      __builtin_memcpy(&v, p, 8);
      w = GTX_U(v);
    }
    else
      for (int32_t k = 0; b.ip + k < b.in_len; ++k)
        w |= static_cast<uint64_t>(GTX_U(static_cast<uint32_t>(b.in[b.ip + k]))) << (8 * k);
    b.buf |= w << b.cnt;
  }
  b.ip += static_cast<int32_t>((63u - b.cnt) >> 3); // (behind the stream: zeros come in, and `overrun` says so before they count)
  b.cnt |= 56u;
}
GTX_DEV bool overrun(Bits const & b) { return (static_cast<int64_t>(b.ip) - b.in_len) * 8 > static_cast<int64_t>(b.cnt); }
GTX_DEV uint32_t take(Bits & b, uint32_t n)
{
  uint32_t const v = static_cast<uint32_t>(b.buf) & ((1u << n) - 1u);
  b.buf >>= n;
  b.cnt -= n;
  return v;
}

// One symbol (needs 15 bits in the buffer): the first-level table, else the canonical walk.  0xFFFF: no code of the set.
template <class W>
GTX_DEV uint32_t decode_sym(uint16_t const * tab, uint32_t tab_bits, uint16_t const * count, uint16_t const * sorted, Bits & b)
{
  uint32_t const e = GTX_U(static_cast<uint32_t>(tab[static_cast<uint32_t>(b.buf) & ((1u << tab_bits) - 1u)]));
  if (e)
  {
    take(b, e & 15u);
    return e >> 4;
  }
  uint32_t code = 0, first = 0, index = 0, bits = static_cast<uint32_t>(b.buf);
  for (uint32_t len = 1; len <= 15; ++len)
  {
    code |= bits & 1u;
    bits >>= 1;
    uint32_t const cnt = GTX_U(static_cast<uint32_t>(count[len]));
    if (code < first + cnt)
    {
      take(b, len);
      return GTX_U(static_cast<uint32_t>(sorted[index + (code - first)]));
    }
    index += cnt;
    first = (first + cnt) << 1;
    code <<= 1;
  }
  return 0xFFFFu;
}

// count[] / sorted[] / first-level table of the canonical code with lengths lens[0, n).  false: over-subscribed, or incomplete
// (a code of one symbol of length 1 passes where `single_ok`, as in zlib).  A set without any symbol decodes nothing.
template <class W>
GTX_DEV bool build_code(uint8_t const * lens, uint32_t n, bool single_ok, uint16_t * count, uint16_t * sorted, uint16_t * tab, uint32_t tab_bits)
{
  W::lds_sync(); // lens is written
  // lane l counts the symbols of length l and sorts them behind those of the shorter lengths
  W::lanes([&](uint32_t l) {
    if (l < 16)
    {
      uint32_t c = 0;
      for (uint32_t i = 0; i < n; ++i)
        c += lens[i] == l;
      count[l] = static_cast<uint16_t>(c);
    }
  });
  W::lds_sync();
  int32_t left = 1;
  uint32_t max_len = 0;
  for (uint32_t l = 1; l <= 15; ++l)
  {
    uint32_t const c = GTX_U(static_cast<uint32_t>(count[l]));
    left = (left << 1) - static_cast<int32_t>(c);
    if (left < 0)
      return false;
    if (c)
      max_len = l;
  }
  if (left > 0 && max_len != 0 && !(single_ok && max_len == 1))
    return false;
  W::lanes([&](uint32_t l) {
    if (l >= 1 && l < 16)
    {
      uint32_t at = 0;
      for (uint32_t k = 1; k < l; ++k)
        at += count[k];
      for (uint32_t i = 0; i < n; ++i)
        if (lens[i] == l)
          sorted[at++] = static_cast<uint16_t>(i);
    }
  });
  W::lds_sync();
  W::lanes([&](uint32_t l) {
    for (uint32_t i = l; i < (1u << tab_bits); i += 64)
    {
      uint32_t code = 0, first = 0, index = 0, bits = i, e = 0;
      for (uint32_t len = 1; len <= tab_bits; ++len)
      {
        code |= bits & 1u;
        bits >>= 1;
        uint32_t const cnt = count[len];
        if (code < first + cnt)
        {
          e = (static_cast<uint32_t>(sorted[index + (code - first)]) << 4) | len;
          break;
        }
        index += cnt;
        first = (first + cnt) << 1;
        code <<= 1;
      }
      tab[i] = static_cast<uint16_t>(e);
    }
  });
  W::lds_sync();
  return true;
}

// the batch of tokens to the output
template <class W>
GTX_DEV void flush(InflateWs & ws, uint8_t * out, uint32_t n_tok, bool any_match)
{
  if (n_tok == 0)
    return;
  W::lds_sync();
  W::lanes([&](uint32_t l) {
    if (l < n_tok)
    {
      uint32_t const p = ws.tok_pos[l];
      if (!(p & INFL_TOK_MATCH))
        out[p] = static_cast<uint8_t>(ws.tok_val[l]);
    }
  });
  if (any_match)
  {
    W::mem_sync(); // everything in front of the batch and the batch's literals are in memory
    uint32_t unfenced_lo = 0xFFFFFFFFu; // where the first match written since the last fence begins
    for (uint32_t t = 0; t < n_tok; ++t)
    {
      uint32_t const p = GTX_U(ws.tok_pos[t]);
      if (!(p & INFL_TOK_MATCH))
        continue;
      uint32_t const v = GTX_U(ws.tok_val[t]);
      uint32_t const pos = p & ~INFL_TOK_MATCH, len = v >> 16, dist = (v & 0xFFFFu) + 1u;
      uint32_t const src = pos - dist, src_end = src + (len < dist ? len : dist);
      if (src_end > unfenced_lo)
      {
        W::mem_sync();
        unfenced_lo = 0xFFFFFFFFu;
      }
      bool const repeats = dist < len;
      W::lanes([&](uint32_t l) {
        for (uint32_t i = l; i < len; i += 64)
          out[pos + i] = out[src + (repeats ? i % dist : i)];
      });
      if (pos < unfenced_lo)
        unfenced_lo = pos;
    }
  }
  W::lds_sync(); // (the tokens are read: the walk may overwrite them)
}

// multiplication modulo the gzip polynomial, reflected: bit 31 is x^0 (zlib's multmodp)
GTX_DEV uint32_t crc_mul(uint32_t a, uint32_t b)
{
  uint32_t p = 0;
  for (uint32_t i = 0; i < 32; ++i)
  {
    p ^= b & (0u - ((a >> (31 - i)) & 1u));
    b = (b >> 1) ^ (0xEDB88320u & (0u - (b & 1u)));
  }
  return p;
}

// CRC-32 of out[0, n): lane l takes the l-th slice (its register starts at 0, lane 0's at ~0), moves it to the end of the data by
// multiplying with x^(8 * bytes behind the slice), and the lanes' values are added
template <class W>
GTX_DEV uint32_t crc32_wave(InflateWs & ws, uint8_t const * out, uint32_t n)
{
  uint32_t const slice = (n + 63u) / 64u;
  W::lanes([&](uint32_t l) {
    uint32_t const b = l * slice < n ? l * slice : n, e = b + slice < n ? b + slice : n;
    uint32_t c = l == 0 ? 0xFFFFFFFFu : 0u;
    for (uint32_t i = b; i < e; ++i)
    {
      c ^= out[i];
      for (uint32_t k = 0; k < 8; ++k)
        c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
    }
    uint32_t x = 0x80000000u, q = 0x00800000u; // x^0, x^8
    for (uint32_t behind = n - e; behind; behind >>= 1)
    {
      if (behind & 1u)
        x = crc_mul(x, q);
      q = crc_mul(q, q);
    }
    ws.tok_val[l] = crc_mul(c, x);
  });
  W::lds_sync();
  uint32_t c = 0;
  for (uint32_t l = 0; l < 64; ++l)
    c ^= GTX_U(ws.tok_val[l]);
  W::lds_sync();
  return ~c;
}

// the stream in[0, in_len) into exactly out_len bytes at out
template <class W>
GTX_DEV uint32_t inflate_stream(InflateWs & ws, uint8_t const * in, uint32_t in_len, uint8_t * out, uint32_t out_len)
{
  Bits b{in, static_cast<int32_t>(in_len), 0, 0, 0};
  uint32_t op = 0, n_tok = 0;
  bool any_match = false;
  for (bool last = false; !last;)
  {
    if (overrun(b))
      return INFL_BAD_STREAM;
    refill<W>(b);
    last = take(b, 1) != 0;
    uint32_t const type = take(b, 2);
    if (type == 3)
      return INFL_BAD_STREAM;
    if (type == 0)
    {
      // stored: back to the byte boundary, LEN, NLEN, bytes
      take(b, b.cnt & 7u);
      b.ip -= static_cast<int32_t>(b.cnt >> 3); // the whole bytes still in the buffer go back
      b.buf = 0;
      b.cnt = 0;
      if (b.ip < 0 || b.ip + 4 > b.in_len)
        return INFL_BAD_STREAM;
      uint32_t const h0 = GTX_U(static_cast<uint32_t>(in[b.ip])), h1 = GTX_U(static_cast<uint32_t>(in[b.ip + 1])),
                     h2 = GTX_U(static_cast<uint32_t>(in[b.ip + 2])), h3 = GTX_U(static_cast<uint32_t>(in[b.ip + 3]));
      uint32_t const len = h0 | (h1 << 8), nlen = h2 | (h3 << 8);
      b.ip += 4;
      if ((len ^ nlen) != 0xFFFFu || len > static_cast<uint32_t>(b.in_len - b.ip))
        return INFL_BAD_STREAM;
      if (len > out_len - op)
        return INFL_LONG;
      flush<W>(ws, out, n_tok, any_match);
      n_tok = 0;
      any_match = false;
      uint8_t const * from = in + b.ip;
      uint8_t * to = out + op;
      W::lanes([&](uint32_t l) {
        for (uint32_t i = l; i < len; i += 64)
          to[i] = from[i];
      });
      b.ip += static_cast<int32_t>(len);
      op += len;
      continue;
    }
    if (type == 1)
    {
      W::lds_sync(); // (tokens and tables of the block before are read)
      W::lanes([&](uint32_t l) {
        for (uint32_t i = l; i < 288 + 32; i += 64)
          ws.lens[i] = static_cast<uint8_t>(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5);
      });
      if (!build_code<W>(ws.lens, 288, true, ws.lit_count, ws.lit_sorted, ws.lit_tab, INFL_LIT_BITS) ||
          !build_code<W>(ws.lens + 288, 32, true, ws.dist_count, ws.dist_sorted, ws.dist_tab, INFL_DIST_BITS))
        return INFL_BAD_STREAM;
    }
    else
    {
      // dynamic: HLIT, HDIST, HCLEN, the code-length code, then the lengths of both alphabets in one run
      uint32_t const hlit = take(b, 5) + 257u, hdist = take(b, 5) + 1u, hclen = take(b, 4) + 4u;
      if (hlit > 286 || hdist > 30)
        return INFL_BAD_STREAM;
      W::lds_sync();
      W::lanes([&](uint32_t l) {
        if (l < 19)
          ws.lens[l] = 0;
      });
      W::lds_sync();
      for (uint32_t i = 0; i < hclen; ++i)
      {
        if (b.cnt < 3)
          refill<W>(b);
        uint32_t const v = take(b, 3);
        // 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15
        uint32_t const at = i < 3 ? 16 + i : i == 3 ? 0 : (i & 1u) ? 8 - ((i - 3) >> 1) : 8 + ((i - 4) >> 1);
        GTX_LEAD ws.lens[at] = static_cast<uint8_t>(v);
      }
      // (the code-length code: 7 bits at most; its table and canonical form lie where the distance code's will)
      if (!build_code<W>(ws.lens, 19, false, ws.dist_count, ws.dist_sorted, ws.dist_tab, 7) || GTX_U(static_cast<uint32_t>(ws.dist_count[0])) == 19)
        return INFL_BAD_STREAM;
      uint32_t const total = hlit + hdist;
      uint32_t prev = 0;
      for (uint32_t i = 0; i < total;)
      {
        if (overrun(b))
          return INFL_BAD_STREAM;
        refill<W>(b);
        uint32_t const sym = decode_sym<W>(ws.dist_tab, 7, ws.dist_count, ws.dist_sorted, b);
        if (sym < 16)
        {
          GTX_LEAD ws.lens[i] = static_cast<uint8_t>(sym);
          prev = sym;
          ++i;
          continue;
        }
        if (sym > 18)
          return INFL_BAD_STREAM;
        uint32_t rep, val = 0;
        if (sym == 16)
        {
          if (i == 0)
            return INFL_BAD_STREAM;
          val = prev;
          rep = 3 + take(b, 2);
        }
        else if (sym == 17)
          rep = 3 + take(b, 3);
        else
          rep = 11 + take(b, 7);
        if (i + rep > total)
          return INFL_BAD_STREAM;
        W::lanes([&](uint32_t l) {
          for (uint32_t k = l; k < rep; k += 64)
            ws.lens[i + k] = static_cast<uint8_t>(val);
        });
        prev = val;
        i += rep;
      }
      W::lds_sync();
      if (GTX_U(static_cast<uint32_t>(ws.lens[256])) == 0) // no end-of-block code
        return INFL_BAD_STREAM;
      // (the distance lengths first: they lie behind the literal / length ones, and building the latter's code does not move them)
      if (!build_code<W>(ws.lens + hlit, hdist, true, ws.dist_count, ws.dist_sorted, ws.dist_tab, INFL_DIST_BITS) ||
          !build_code<W>(ws.lens, hlit, true, ws.lit_count, ws.lit_sorted, ws.lit_tab, INFL_LIT_BITS))
        return INFL_BAD_STREAM;
      if (GTX_U(static_cast<uint32_t>(ws.lit_count[0])) == hlit)
        return INFL_BAD_STREAM;
    }
    // ---- symbols of the block ----
    for (;;)
    {
      if (overrun(b))
        return INFL_BAD_STREAM;
      refill<W>(b);
      uint32_t const sym = decode_sym<W>(ws.lit_tab, INFL_LIT_BITS, ws.lit_count, ws.lit_sorted, b);
      if (sym < 256)
      {
        if (op >= out_len)
          return INFL_LONG;
        GTX_LEAD
        {
          ws.tok_pos[n_tok] = op;
          ws.tok_val[n_tok] = sym;
        }
        ++op;
      }
      else if (sym == 256)
        break;
      else
      {
        if (sym >= 286)
          return INFL_BAD_STREAM;
        uint32_t const ls = sym - 257u;
        uint32_t const len = len_base(ls) + take(b, len_extra(ls));
        // (at most 15 + 5 bits are gone: 36 left, a distance takes 15 + 13)
        uint32_t const ds = decode_sym<W>(ws.dist_tab, INFL_DIST_BITS, ws.dist_count, ws.dist_sorted, b);
        if (ds >= 30)
          return INFL_BAD_STREAM;
        uint32_t const dist = dist_base(ds) + take(b, dist_extra(ds));
        if (dist > op)
          return INFL_BAD_STREAM;
        if (len > out_len - op)
          return INFL_LONG;
        GTX_LEAD
        {
          ws.tok_pos[n_tok] = op | INFL_TOK_MATCH;
          ws.tok_val[n_tok] = (len << 16) | (dist - 1u);
        }
        any_match = true;
        op += len;
      }
      if (++n_tok == INFL_TOKENS)
      {
        flush<W>(ws, out, n_tok, any_match);
        n_tok = 0;
        any_match = false;
      }
    }
    if (overrun(b))
      return INFL_BAD_STREAM;
  }
  flush<W>(ws, out, n_tok, any_match);
  return op == out_len ? INFL_OK : INFL_SHORT;
}
} // namespace inflate_dev

// One member of a batch: the descriptor is checked against the batch's buffers (in_size bytes of streams at in, out_size bytes
// at out), the stream inflated, and the output's CRC-32 compared with the member's.  Returns the member's status.
template <class W>
GTX_DEV uint32_t inflate_member_dev(InflateWs & ws, uint8_t const * in, uint64_t in_size, InflateMember const & m, uint8_t * out, uint64_t out_size,
                                    bool check_crc)
{
  if (m.in_off > in_size || m.in_len > in_size - m.in_off || m.in_len > 0x7FFFFFF0u || m.out_len > INFL_MAX_OUT || m.out_off > out_size ||
      m.out_len > out_size - m.out_off)
    return INFL_BAD_MEMBER;
  uint8_t * const o = out + m.out_off;
  uint32_t const st = inflate_dev::inflate_stream<W>(ws, in + m.in_off, m.in_len, o, m.out_len);
  if (st != INFL_OK || !check_crc)
    return st;
  W::mem_sync(); // the last tokens' stores
  return inflate_dev::crc32_wave<W>(ws, o, m.out_len) == m.crc32 ? INFL_OK : INFL_CRC;
}
} // namespace gtx
