// k_pack.hip — export: quantize + pack into 2 / 4 / 8-bit fields (vsiq_quantize_pack_f32)
// and the inverse, unpack + dequantize (vsiq_unpack_dequant); layout in include/vsiq.h.
//
// Both kernels run one flat grid over SLOTS: a slot is 16 consecutive elements of one row
// (slots per row = ceil(rowlen / 16)), and a lane owns one slot -- four groups of 4
// elements on the input side, bits/2 whole dwords on the packed side (row starts in
// `packed` are dword-aligned by construction).  A workgroup therefore takes 256 slots of
// however many rows they span: 64 rows of 27 elements are 128 slots, one workgroup.  A
// lane's row is slot / slots-per-row; with per-row qparams each lane reads its own row's.
// No reduction, no atomics, no workspace, no LDS.
#include "dispatch.cuh"

namespace vsiq {

constexpr int kSlotElems = 16;

struct PackArgs {
  int64_t rows, rowlen;
  uint32_t spr;          // slots per row
  uint32_t nslots;       // rows * spr
  uint32_t row_dwords;   // dwords of a packed row
  int qmin;
  float lo, hi;
  int zp_round;
  const double *scale, *zp;   // f64 [1] or [rows]; zp nullable: 0
};

// the lane's slot -> (row, slot of the row); past the grid's end the last slot (loads are
// issued unconditionally, stores predicated on `in`)
struct Slot {
  uint32_t row, t;
  bool in;
};
__device__ __forceinline__ Slot slot_of(uint32_t nslots, uint32_t spr) {
  const uint32_t j = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  Slot s;
  s.in = j < nslots;
  const uint32_t jc = s.in ? j : nslots - 1;
  s.row = jc / spr;
  s.t = jc - s.row * spr;
  return s;
}

// the 4 code bytes of a group (the forward kernels' `codes` bytes) -> 4 fields of BITS:
// field = code - qmin, elements past the row's end (j >= nv) give 0
template <int BITS>
__device__ __forceinline__ uint32_t pack_fields(uint32_t c, int qmin, int nv) {
  constexpr uint32_t fm = (1u << BITS) - 1u;
  uint32_t o = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t f = (((c >> (8 * j)) & 0xffu) - (uint32_t)qmin) & fm;
    o |= (j < nv ? f : 0u) << (BITS * j);
  }
  return o;
}

// PERROW: one qparam pair per row (vector loads of the lane's row's), else one pair for
// the tensor (scalar loads after the x loads are issued, as K1).  WIDE: every slot is
// whole (rowlen % 16 == 0) and `packed` 16-byte aligned -> one store of bits/2 dwords.
template <int BITS, bool VEC, bool NT, bool PERROW, bool WIDE>
__global__ __launch_bounds__(kBlock) void k_quantize_pack(const float *__restrict__ x,
                                                          uint32_t *__restrict__ packed,
                                                          float *__restrict__ qparams_out, PackArgs a) {
  constexpr int ND = BITS / 2;   // dwords per slot
  const Slot sl = slot_of(a.nslots, a.spr);
  const float *xr = x + (int64_t)sl.row * a.rowlen;
  const int64_t ng = cdiv(a.rowlen, 4);
  const int64_t g0 = 4 * (int64_t)sl.t;
  f4 v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = load_group_c<VEC, NT>(xr, g0 + k, ng, a.rowlen);
  const uint32_t qrow = PERROW ? sl.row : 0u;
  const QPSrc src{nullptr, a.scale + qrow, a.zp ? a.zp + qrow : nullptr, 0.0, 0.0, a.lo, a.hi, a.zp_round, 0};
  const QP p = load_qp<!PERROW>(src);
  uint32_t w[ND] = {};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const GroupOut go = fq_out_flat<VEC, true, false>(v[k], p, g0 + k, a.rowlen);
    const int nv = g0 + k < ng ? valid_in_group(g0 + k, a.rowlen) : 0;
    const uint32_t f = pack_fields<BITS>(go.c, a.qmin, nv);   // 4 * BITS bits
    w[(k * 4 * BITS) / 32] |= f << ((k * 4 * BITS) % 32);
  }
  if (!sl.in) return;
  if (sl.t == 0 && (PERROW || sl.row == 0)) {   // the export's qparams: the fp32 pair used
    qparams_out[2 * qrow] = p.s;
    qparams_out[2 * qrow + 1] = p.z;
  }
  const int64_t d0 = (int64_t)sl.row * a.row_dwords + (int64_t)sl.t * ND;
  if constexpr (WIDE && ND == 4) {
    typedef uint32_t u4 __attribute__((ext_vector_type(4)));
    u4 o;
    o.x = w[0]; o.y = w[1]; o.z = w[2]; o.w = w[3];
    *reinterpret_cast<u4 *>(packed + d0) = o;
  } else if constexpr (WIDE && ND == 2) {
    u2 o;
    o.x = w[0]; o.y = w[1];
    *reinterpret_cast<u2 *>(packed + d0) = o;
  } else {
#pragma unroll
    for (int d = 0; d < ND; ++d)   // the row's last slot may own fewer than ND dwords
      if (sl.t * ND + d < a.row_dwords) packed[d0 + d] = w[d];
  }
}

struct UnpackArgs {
  int64_t rows, rowlen;
  uint32_t spr, nslots, row_dwords;
  int qmin;
  int perrow;
};

// y (nullable) and codes (nullable) are kernel-uniform branches.  VEC: rowlen % 4 == 0,
// y aligned for 4-element stores and codes for dword stores.
template <int BITS, typename T, bool VEC, bool NT>
__global__ __launch_bounds__(kBlock) void k_unpack_dequant(const uint32_t *__restrict__ packed,
                                                           T *__restrict__ y, uint8_t *__restrict__ codes,
                                                           const float *__restrict__ qparams, UnpackArgs a) {
  constexpr int ND = BITS / 2;
  constexpr uint32_t fm = (1u << BITS) - 1u;
  const Slot sl = slot_of(a.nslots, a.spr);
  const int64_t rd0 = (int64_t)sl.row * a.row_dwords;
  uint32_t w[ND];
#pragma unroll
  for (int d = 0; d < ND; ++d) {   // clamped into the row: unconditional loads
    const uint32_t i = sl.t * ND + d;
    const uint32_t *q = packed + rd0 + (i < a.row_dwords ? i : a.row_dwords - 1);
    w[d] = NT ? __builtin_nontemporal_load(q) : *q;
  }
  const uint32_t qrow = a.perrow ? sl.row : 0u;
  const float s = qparams[2 * qrow], z = qparams[2 * qrow + 1];
  if (!sl.in) return;
  const int64_t ng = cdiv(a.rowlen, 4);
  const int64_t g0 = 4 * (int64_t)sl.t;
  T *yr = y ? y + (int64_t)sl.row * a.rowlen : nullptr;
  uint8_t *cr = codes ? codes + (int64_t)sl.row * a.rowlen : nullptr;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t f = w[(k * 4 * BITS) / 32] >> ((k * 4 * BITS) % 32);
    GroupOut go;
    float yv[4];
    go.c = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int q = (int)((f >> (BITS * j)) & fm) + a.qmin;
      yv[j] = ((float)q - z) * s;   // the forward kernels' last two operations
      go.c |= ((uint32_t)q & 0xffu) << (8 * j);
    }
    go.o.x = yv[0]; go.o.y = yv[1]; go.o.z = yv[2]; go.o.w = yv[3];
    if (g0 + k >= ng) break;
    if (yr) store_group<VEC, NT>(yr, g0 + k, a.rowlen, go.o);
    if (cr) {
      if (VEC) reinterpret_cast<uint32_t *>(cr)[g0 + k] = go.c;
      else
        for (int j = 0; j < valid_in_group(g0 + k, a.rowlen); ++j) cr[4 * (g0 + k) + j] = (uint8_t)(go.c >> (8 * j));
    }
  }
}

inline bool pack_bits_ok(int bits) { return bits == 2 || bits == 4 || bits == 8; }

inline int64_t packed_row_dwords(int64_t rowlen, int bits) { return cdiv(rowlen * bits, 32); }

// shared argument checks; on success the slot grid's geometry
inline int pack_geometry(int64_t rows, int64_t rowlen, int64_t nq, int bits, uint32_t *spr, uint32_t *nslots,
                         uint32_t *row_dwords) {
  if (rows < 0 || rowlen <= 0 || !pack_bits_ok(bits)) return VSIQ_E_ARG;
  if (rows > 0 && nq != 1 && nq != rows) return VSIQ_E_ARG;
  const int64_t s = cdiv(rowlen, kSlotElems);
  if (s > 0x3fffffffLL || (rows > 0 && s > 0xffffff00LL / rows)) return VSIQ_E_ARG;   // 32-bit slot and dword indices
  *spr = (uint32_t)s;
  *nslots = (uint32_t)(rows * s);
  *row_dwords = (uint32_t)packed_row_dwords(rowlen, bits);
  return 0;
}

}  // namespace vsiq

using namespace vsiq;

extern "C" {

int64_t vsiq_packed_row_bytes(int64_t rowlen, int bits) {
  if (rowlen < 0 || !pack_bits_ok(bits)) return -1;
  return 4 * packed_row_dwords(rowlen, bits);
}

int vsiq_quantize_pack_f32(const float *x, void *packed, float *qparams_out, int64_t rows, int64_t rowlen,
                           const double *scale, const double *zp, int64_t nq, int zp_round, int qmin, int qmax,
                           int bits, void *stream) {
  PackArgs a{};
  if (const int e = pack_geometry(rows, rowlen, nq, bits, &a.spr, &a.nslots, &a.row_dwords)) return e;
  if (qmin > qmax || (int64_t)qmax - (int64_t)qmin + 1 > (int64_t)1 << bits) return VSIQ_E_ARG;
  if (rows == 0) return 0;
  if (!x || !packed || !qparams_out || !scale) return VSIQ_E_ARG;
  if (!aligned4(packed)) return VSIQ_E_ALIGN;
  a.rows = rows; a.rowlen = rowlen; a.qmin = qmin; a.lo = (float)qmin; a.hi = (float)qmax;
  a.zp_round = zp_round; a.scale = scale; a.zp = zp;
  const bool vec = rowlen % 4 == 0 && aligned16(x);
  const bool nt = g_tune.nontemporal != 0;
  const bool wide = rowlen % kSlotElems == 0 && aligned16(packed);
  const dim3 grid((unsigned)cdiv(a.nslots, kBlock)), block(kBlock);
  hipStream_t st = (hipStream_t)stream;
  uint32_t *pk = (uint32_t *)packed;
  with_int<2, 4, 8>(bits, [&](auto B) {
    with_vec_nt(vec, nt, [&](auto V, auto N) {
      with_bool2(nq != 1, wide, [&](auto P, auto W) {
        hipLaunchKernelGGL((k_quantize_pack<decltype(B)::value, decltype(V)::value, decltype(N)::value,
                                            decltype(P)::value, decltype(W)::value>),
                           grid, block, 0, st, x, pk, qparams_out, a);
      });
    });
  });
  return launch_rc();
}

int vsiq_unpack_dequant(const void *packed, void *y, void *codes, int64_t rows, int64_t rowlen,
                        const float *qparams, int64_t nq, int qmin, int bits, int dtype, void *stream) {
  UnpackArgs a{};
  if (const int e = pack_geometry(rows, rowlen, nq, bits, &a.spr, &a.nslots, &a.row_dwords)) return e;
  if (!dtype_ok(dtype)) return VSIQ_E_ARG;
  if (rows == 0) return 0;
  if (!packed || !qparams) return VSIQ_E_ARG;
  if (!aligned4(packed)) return VSIQ_E_ALIGN;
  if (!y && !codes) return 0;
  a.rows = rows; a.rowlen = rowlen; a.qmin = qmin; a.perrow = nq != 1;
  const bool nt = g_tune.nontemporal != 0;
  const dim3 grid((unsigned)cdiv(a.nslots, kBlock)), block(kBlock);
  hipStream_t st = (hipStream_t)stream;
  const uint32_t *pk = (const uint32_t *)packed;
  uint8_t *c = (uint8_t *)codes;
  with_int<2, 4, 8>(bits, [&](auto B) {
    with_dtype(dtype, [&](auto D) {
      using T = typename decltype(D)::type;
      const bool vec = rowlen % 4 == 0 && (!y || aligned_vec<T>(y)) && (!c || aligned4(c));
      with_vec_nt(vec, nt, [&](auto V, auto N) {
        hipLaunchKernelGGL((k_unpack_dequant<decltype(B)::value, T, decltype(V)::value, decltype(N)::value>), grid,
                           block, 0, st, pk, (T *)y, c, qparams, a);
      });
    });
  });
  return launch_rc();
}

}  // extern "C"
