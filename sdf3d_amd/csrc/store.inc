// store.inc -- what a pixel is stored as: the framebuffer formats and the TILES
// wire-format encoder.
// Included by render_kernel.inc inside namespace SDF_NS (the order of the layers
// is there); no guards, includes nothing.

// ---- framebuffer formats (sdf_abi.h sdf_format) ----------------------------
// RGBA8 = trunc(min(max(c,0),1) * 255 + 0.5) with NaN -> 0, the multiply and
// add rounded separately (__fmul_rn / __fadd_rn) in both precisions.
__device__ __forceinline__ unsigned to_unorm8(float c) {
  const float q = fminf(fmaxf(c, 0.0f), 1.0f);
  return (unsigned)__fadd_rn(__fmul_rn(q, 255.0f), 0.5f);
}
__device__ __forceinline__ void store_pixel(int format, void* out, size_t o, float4 c) {
  if (format == SDF_FORMAT_RGBA8) {
    const unsigned u = to_unorm8(c.x) | (to_unorm8(c.y) << 8) | (to_unorm8(c.z) << 16) |
                       (to_unorm8(c.w) << 24);
    reinterpret_cast<unsigned*>(out)[o] = u;
  } else if (format == SDF_FORMAT_RGBA16F) {
    const _Float16 h[4] = {(_Float16)c.x, (_Float16)c.y, (_Float16)c.z, (_Float16)c.w};
    uint2 u;
    __builtin_memcpy(&u, h, 8);
    reinterpret_cast<uint2*>(out)[o] = u;
  } else if (format == SDF_FORMAT_RGB32F) {
    float* q = reinterpret_cast<float*>(out) + 3 * o;
    q[0] = c.x;
    q[1] = c.y;
    q[2] = c.z;
  } else {
    reinterpret_cast<float4*>(out)[o] = c;
  }
}

// ---- TILES wire format encoder (sdf_abi.h SDF_FORMAT_TILES) ----------------
// One wave = one 8x8 tile (lane j = pixel 8 * row + column), all 64 lanes
// present; lanes outside the frame carry u = 0 and z = 0.  Neighbours of a
// pixel in the frame are in the frame, so residuals never read those lanes.
// The head goes to its fixed place in the stream, the data to the tile's
// worst-case slot in the scratch area; tiles.hip then compacts the slots into
// the stream in tile order (an allocator shared by every wave would
// serialise on one address).
// Per channel: the gradient residual as the horizontal difference h = u -
// left (DPP row shift; 0 left of the tile) minus the row above's h (one
// ds_bpermute; 0 above the tile), i.e. u - L - U + UL in two neighbour
// reads; zigzag; then one 64 x 64 bit transpose (wave_bits.h) puts plane b
// in lane b and a ballot of the non-zero planes gives the width w (instead
// of a ballot + two v_writelane per plane and a 6-step wave OR).  The base
// width b <= w is the cheapest in bits of w and w - 1 .. w - 12 with an
// escape for the pixels wider than b, all candidates at once in lanes (a
// suffix OR of the planes and a min-reduction: ~30 VALU per channel, where a
// loop of one ballot per candidate spent ~200 mostly scalar instructions and
// 9% of the whole render); the
// escaped pixels' high bits are packed into the tile's bitstream with LDS
// atomic ORs (mbcnt gives each its field index), and so are the base bits,
// pixel by pixel (ABI 10: each lane's low b bits at bit j b; the planes serve
// only the width search, and the decoder loads its bits directly instead of
// transposing: rank 0's N = 8 decode 0.0408 -> 0.0393 ms, the encoder's cost
// unchanged, profiles/r04_lane_major.json).
__device__ __forceinline__ uint32_t ordered_bits(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? (u ^ 0x7fffffffu) : u;
}
// inside each 16-lane DPP row: lane i := OR of lanes i.. (row_shl), max of
// lanes ..i (row_shr); zeros shifted in, so each step is one v_or / v_max
// with a DPP operand
__device__ __forceinline__ uint32_t row_suffix_or(uint32_t x) {
  x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x101, 0xF, 0xF, true);
  x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x102, 0xF, 0xF, true);
  x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x104, 0xF, 0xF, true);
  x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x108, 0xF, 0xF, true);
  return x;
}
__device__ __forceinline__ uint32_t row_prefix_max(uint32_t x) {
  x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xF, 0xF, true));
  x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xF, 0xF, true));
  x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xF, 0xF, true));
  x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xF, 0xF, true));
  return x;
}
__device__ __forceinline__ void store_tiles(void* out, int ntiles, int tile, int lane, bool valid,
                                            float4 c) {
  uint8_t* const base = reinterpret_cast<uint8_t*>(out);
  const int col = lane & 7;
  const TransposeLanes TL(lane);
  const int up = ((lane - 8) & 63) << 2;   // ds_bpermute address of lane - 8
  const int tl = lane & 31;                 // plane index within a half
  const bool low_row = (lane & 16) == 0;    // lanes 0..15, 32..47
  const uint32_t cost0 = 64u * (uint32_t)tl + 72u;
  uint32_t first[3], zc[3];
  int bw[3], wd[3];
  uint64_t esc[3];
#pragma unroll
  for (int ch = 0; ch < 3; ch++) {
    const float v = ch == 0 ? c.x : (ch == 1 ? c.y : c.z);
    const uint32_t u = valid ? ordered_bits(v) : 0u;
    // lane - 1 inside the 16-lane DPP row (row_shr:1, 0 shifted in)
    const uint32_t left = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)u, 0x111, 0xF, 0xF, true);
    const uint32_t h = u - (col ? left : 0u);
    const uint32_t habove = (uint32_t)__builtin_amdgcn_ds_bpermute(up, (int)h);
    const int32_t r = (int32_t)(h - (lane >= 8 ? habove : 0u));   // mod 2^32
    uint32_t zz = ((uint32_t)r << 1) ^ (uint32_t)(r >> 31);      // zigzag
    if (lane == 0 || !valid) zz = 0u;
    first[ch] = __builtin_amdgcn_readfirstlane(u);
    zc[ch] = zz;
  }
  if (__builtin_amdgcn_ballot_w64(((zc[0] | zc[2]) >> 16) != 0u) == 0) {
    // Narrow tile (channels 0 and 2 under 16 bits, most tiles): ONE transpose
    // of (z0 | z2 << 16, z1) -- lanes 0..15 get planes 0..15 of channel 0,
    // 16..31 those of channel 2, 32..63 planes 0..31 of channel 1 -- and one
    // base-width search, each 16-lane DPP row a channel (channel 1 two rows)
    uint32_t a = zc[0] | (zc[2] << 16), b = zc[1];
    transpose64(a, b, TL);
    const uint64_t nz = __builtin_amdgcn_ballot_w64((a | b) != 0u);
    const uint32_t nz0 = (uint32_t)nz & 0xFFFFu, nz2 = (uint32_t)nz >> 16, nz1 = (uint32_t)(nz >> 32);
    wd[0] = nz0 ? 32 - __builtin_clz(nz0) : 0;
    wd[2] = nz2 ? 32 - __builtin_clz(nz2) : 0;
    wd[1] = nz1 ? 32 - __builtin_clz(nz1) : 0;
    const int t = lane < 32 ? (lane & 15) : lane - 32;   // plane of its channel
    const int w = lane < 16 ? wd[0] : (lane < 32 ? wd[2] : wd[1]);
    uint32_t sa = row_suffix_or(a), sb = row_suffix_or(b);
    const uint32_t ra48 = (uint32_t)__builtin_amdgcn_readlane((int)sa, 48);
    const uint32_t rb48 = (uint32_t)__builtin_amdgcn_readlane((int)sb, 48);
    const bool ch1_low = (lane & 48) == 32;   // channel 1's planes 0..15 add 16..31
    sa |= ch1_low ? ra48 : 0u;
    sb |= ch1_low ? rb48 : 0u;
    const uint32_t n = (uint32_t)(__builtin_popcount(sa) + __builtin_popcount(sb));
    const uint32_t cost = 64u * (uint32_t)t + 72u + (uint32_t)(w - t) * n;
    uint32_t nkey = t < w && t >= w - kEscapeWindow ? ~((cost << 6) | (uint32_t)(63 - t)) : 0u;
    nkey = row_prefix_max(nkey);
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
      const int pbase = ch == 0 ? 0 : (ch == 2 ? 16 : 32);
      const uint32_t kmax =
          ch == 1 ? max((uint32_t)__builtin_amdgcn_readlane((int)nkey, 47),
                        (uint32_t)__builtin_amdgcn_readlane((int)nkey, 63))
                  : (uint32_t)__builtin_amdgcn_readlane((int)nkey, pbase + 15);
      const uint32_t kmin = ~kmax;
      int bsel = wd[ch];
      uint64_t bmask = 0ull;
      if ((kmin >> 6) < 64u * (uint32_t)wd[ch]) {
        bsel = 63 - (int)(kmin & 63u);
        bmask = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)sa, pbase + bsel) |
                (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)sb, pbase + bsel) << 32;
      }
      bw[ch] = bsel;
      esc[ch] = bmask;
    }
  } else {
    // Two channels per transpose: lane j holds (z_j of channel A, z_j of B),
    // so lane p < 32 gets plane p of A and lane 32 + p plane p of B (pixels
    // 0..31 in the low word, 32..63 in the high); channel 2 pairs with zeros.
  #pragma unroll
    for (int g = 0; g < 2; g++) {
      const int cA = 2 * g, cB = 2 * g + 1;   // cB = 3: none
      uint32_t a = zc[cA], b = g == 0 ? zc[1] : 0u;
      transpose64(a, b, TL);
      const uint64_t nz = __builtin_amdgcn_ballot_w64((a | b) != 0u);
      const uint32_t nzA = (uint32_t)nz, nzB = (uint32_t)(nz >> 32);
      const int wA = nzA ? 32 - __builtin_clz(nzA) : 0, wB = nzB ? 32 - __builtin_clz(nzB) : 0;
      const int w = lane < 32 ? wA : wB;
      // the cheapest base width: w planes, or t < w planes plus an escape for
      // the n(t) pixels wider than t (their mask, a width byte, w - t bits
      // each), every candidate t in its own lane: the suffix OR of the planes
      // (lanes t.. of the half) is the mask of the pixels wider than t
      // + planes 16..31 of the half (no branch: a readlane inside divergent
      // code may read a lane the branch left undefined)
      uint32_t sa = row_suffix_or(a), sb = row_suffix_or(b);
      const uint32_t ra16 = (uint32_t)__builtin_amdgcn_readlane((int)sa, 16);
      const uint32_t ra48 = (uint32_t)__builtin_amdgcn_readlane((int)sa, 48);
      const uint32_t rb16 = (uint32_t)__builtin_amdgcn_readlane((int)sb, 16);
      const uint32_t rb48 = (uint32_t)__builtin_amdgcn_readlane((int)sb, 48);
      sa |= low_row ? (lane < 32 ? ra16 : ra48) : 0u;
      sb |= low_row ? (lane < 32 ? rb16 : rb48) : 0u;
      const uint32_t n = (uint32_t)(__builtin_popcount(sa) + __builtin_popcount(sb));
      const uint32_t cost = cost0 + (uint32_t)(w - tl) * n;   // 64 t + 72 + (w - t) n
      // candidates t = w - 12 .. w - 1 (t >= 0); the key orders by size, then
      // by the larger t; minimised as its complement (0: no candidate)
      uint32_t nkey = tl < w && tl >= w - kEscapeWindow ? ~((cost << 6) | (uint32_t)(63 - tl)) : 0u;
      nkey = row_prefix_max(nkey);
  #pragma unroll
      for (int hf = 0; hf < 2; hf++) {
        const int ch = hf == 0 ? cA : cB;
        if (ch > 2) break;
        const int wc = hf == 0 ? wA : wB;
        const uint32_t kmin = ~max((uint32_t)__builtin_amdgcn_readlane((int)nkey, 32 * hf + 15),
                                   (uint32_t)__builtin_amdgcn_readlane((int)nkey, 32 * hf + 31));
        int bsel = wc;
        uint64_t bmask = 0ull;
        if ((kmin >> 6) < 64u * (uint32_t)wc) {   // kmin = ~0 (no candidate) never is
          bsel = 63 - (int)(kmin & 63u);
          bmask = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)sa, 32 * hf + bsel) |
                  (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)sb, 32 * hf + bsel) << 32;
        }
        bw[ch] = bsel;
        wd[ch] = wc;
        esc[ch] = bmask;
      }
    }
  }
  // the escapes' bitstream (width bytes, then each escaped channel's fields
  // in pixel order), assembled in this wave's LDS words
  __shared__ uint32_t escape_bits[kWgWaves][kEscapeDwords];
  uint32_t* const eb = escape_bits[threadIdx.x >> 6];
  const int P = (bw[0] < wd[0]) + (bw[1] < wd[1]) + (bw[2] < wd[2]);
  int nbits = 8 * P;
#pragma unroll
  for (int ch = 0; ch < 3; ch++) nbits += (wd[ch] - bw[ch]) * __builtin_popcountll(esc[ch]);
  const int nbq = (nbits + 63) >> 6;   // bitstream qwords
  if (P) {
    if (lane < 2 * nbq) eb[lane] = 0u;
    if (lane + 64 < 2 * nbq) eb[lane + 64] = 0u;
    // pixel-major fields: this pixel's escaped channels' high bits side by
    // side (channel order), starting after the fields of every lower pixel
    uint32_t widths = 0u, o = 8u * (uint32_t)P;
    uint64_t val = 0ull;
    int nb = 0, j = 0;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
      if (bw[ch] == wd[ch]) continue;
      const int d = wd[ch] - bw[ch];
      widths |= (uint32_t)d << (8 * j++);
      const uint64_t m = esc[ch];
      o += (uint32_t)d * __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
                                                   __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
      if ((m >> lane) & 1) {
        val |= (uint64_t)(zc[ch] >> bw[ch]) << nb;   // < 2^d
        nb += d;
      }
    }
    if (nb) {
      const uint32_t s = o & 31, wi = o >> 5;
      atomicOr(&eb[wi], (uint32_t)(val << s));
      if (s + nb > 32) atomicOr(&eb[wi + 1], (uint32_t)((val << s) >> 32));
      if (s + nb > 64) atomicOr(&eb[wi + 2], (uint32_t)(val >> (64 - s)));
    }
    if (lane == 0) atomicOr(&eb[0], widths);
  }
  const int B = bw[0] + bw[1] + bw[2];
  const int nq = B + P + nbq;
  const TilesLayout L(ntiles);
  if (lane == 0)
    reinterpret_cast<uint4*>(base + L.head)[tile] =
        make_uint4((uint32_t)(bw[0] | bw[1] << 6 | bw[2] << 12 | nq << 18 |
                              (bw[0] < wd[0]) << 26 | (bw[1] < wd[1]) << 27 |
                              (bw[2] < wd[2]) << 28),
                   first[0], first[1], first[2]);
  // the tile's data to its slot (tiles.hip compacts the slots): base bits,
  // escape masks, bitstream
  uint2* const q = reinterpret_cast<uint2*>(base + L.slots + (size_t)tile * kTilePlaneBytes);
  // the base bits, lane-major: channel c's bw[c] words follow the earlier
  // channels', pixel j's low bw[c] bits at bit j bw[c] (at most two dwords
  // per pixel), OR-ed into this wave's zeroed LDS words, then stored whole
  __shared__ uint2 base_words[kWgWaves][3 * 32];
  uint2* const bq = base_words[threadIdx.x >> 6];
  uint32_t* const bd = reinterpret_cast<uint32_t*>(bq);
  if (lane < B) bq[lane] = make_uint2(0u, 0u);
  if (lane + 64 < B) bq[lane + 64] = make_uint2(0u, 0u);
  uint32_t qb = 0u;   // the channel's first word
#pragma unroll
  for (int ch = 0; ch < 3; ch++) {
    const int b = bw[ch];
    if (b) {
      const uint32_t v = zc[ch] & (0xFFFFFFFFu >> (32 - b));
      const uint32_t off = 64u * qb + (uint32_t)lane * (uint32_t)b;
      const uint32_t wi = off >> 5, sh = off & 31u;
      atomicOr(&bd[wi], v << sh);
      if (sh + (uint32_t)b > 32u) atomicOr(&bd[wi + 1], v >> (32u - sh));
    }
    qb += (uint32_t)b;
  }
  if (lane < B) q[lane] = bq[lane];
  if (lane + 64 < B) q[lane + 64] = bq[lane + 64];
  int k = bw[0] + bw[1] + bw[2];
  if (lane == 0) {
#pragma unroll
    for (int ch = 0; ch < 3; ch++)
      if (bw[ch] < wd[ch]) q[k++] = make_uint2((uint32_t)esc[ch], (uint32_t)(esc[ch] >> 32));
  }
  if (P) {
    uint32_t* const bits = reinterpret_cast<uint32_t*>(q + B + P);
    if (lane < 2 * nbq) bits[lane] = eb[lane];
    if (lane + 64 < 2 * nbq) bits[lane + 64] = eb[lane + 64];
  }
}
// Stream header words 2..15 (sdf_abi.h SDF_FORMAT_TILES): what the channels
// hold and the frame's shading constants, written by tile 0's wave (words 0
// and 1 are tiles_move's)
__device__ __forceinline__ void store_tiles_shade(void* out, const ShadeK& K, int lane) {
  if (lane >= 14) return;
  const float k[10] = {K.lam[0], K.lam[1], K.lam[2], K.dif[0], K.dif[1],
                       K.dif[2], K.ref[0], K.ref[1], K.ref[2], K.shin};
  uint32_t v = 0u;
  if (lane == 0) v = SDF_EXACT ? kTilesShadeExact : kTilesShadeFast;
#pragma unroll
  for (int i = 0; i < 10; i++)
    if (lane == 2 + i) v = __float_as_uint(k[i]);
  reinterpret_cast<uint32_t*>(out)[2 + lane] = v;
}
