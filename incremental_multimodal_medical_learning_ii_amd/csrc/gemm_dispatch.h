// The tile policy of every MFMA contraction, once: which tile a launch of a given kind and shape takes (pick_tile), and the two
// launchers that act on it — launch_gemm_pw for planes operands, launch_gemm for fp32 operands.  Whoever needs to know the tile
// of a launch (the fused column-sum partials, cxrk_gemm_wide_tile) asks pick_tile with the launch's own arguments.
// (Included at the end of gemm_core.h.)
#pragma once
#include <type_traits>

namespace cxrk {

// Planes operands: gemm_pw_kernel<Pw256 / Pw256x64 / Pw64x256 / Pw128>; fp32 operands: wave tiles 4,1 / 1,4 / 2,2 of the
// register-staged kernels (no 256x256 there).
enum Tile { TILE_256, TILE_256x64, TILE_64x256, TILE_128 };
constexpr int tile_rows(Tile t) { return t == TILE_64x256 ? 64 : t == TILE_128 ? 128 : 256; }
constexpr int tile_cols(Tile t) { return t == TILE_256x64 ? 64 : t == TILE_128 ? 128 : 256; }

// The kind of a launch fixes the shortest K loop that gains on the 256x256 tile (use_wide256's min_k) and the narrow tiles it
// may take: the kernels of the others are not compiled.
enum LaunchKind { DENSE, CONV_FPROP, CONV_DGRAD, CONV_WGRAD };
constexpr bool kind_takes(LaunchKind k, Tile t) {
  return t == TILE_256x64 ? k != CONV_WGRAD : t == TILE_64x256 ? (k == DENSE || k == CONV_WGRAD) : true;
}
static inline long kind_min_k(LaunchKind k) { return k == CONV_FPROP ? WIDE_MINK_FPROP : k == CONV_DGRAD ? WIDE_MINK_DGRAD : WIDE_MINK_PLAIN; }

// 256x256 where use_wide256 says it pays; else 256x64 for outputs of <= 64 columns, then 64x256 for <= 64 rows (in this order: a
// 64x64 output takes 256x64), where the kind has them; else 128x128.
static inline Tile pick_tile(LaunchKind kind, int M, int N, long K, int splitk, bool planes) {
  if (use_wide256(M, N, K, splitk, planes, kind_min_k(kind))) return TILE_256;
  if (kind_takes(kind, TILE_256x64) && N <= 64) return TILE_256x64;
  if (kind_takes(kind, TILE_64x256) && M <= 64) return TILE_64x256;
  return TILE_128;
}
// 64-row slabs of fused column-sum partials (EpiParams::colsum_part) a launch over `rows` output rows writes: its row tiling, padded
static inline int colsum_slabs(Tile t, int rows) { return ceil_div(rows, tile_rows(t)) * (tile_rows(t) / 64); }

// A loader's P struct takes different arguments per loader family but the same for every tile of a family: the caller passes a
// maker, `[&](auto tag) { return typename decltype(tag)::type::P{...}; }`, and the launcher calls it with the loader it chose.
template <class L> struct LoaderTag { using type = L; };

// Planes operands, the tile chosen by the policy.  LAT / LBT: loader families <TILE, NW> of gemm_pw.h.
template <LaunchKind KIND, template <int, int> class LAT, template <int, int> class LBT, class MKA, class MKB>
static int launch_gemm_pw(MKA mka, MKB mkb, const EpiParams& ep, int M, int N, int K, int splitk, hipStream_t stream) {
  auto go = [&](auto cfg) {
    using CFG = decltype(cfg);
    using LA = LAT<CFG::TM, CFG::NW>; using LB = LBT<CFG::TN, CFG::NW>;
    return launch_gemm_pw<CFG, LA, LB>(mka(LoaderTag<LA>{}), mkb(LoaderTag<LB>{}), ep, M, N, K, splitk, stream);
  };
  const Tile t = pick_tile(KIND, M, N, K, splitk, true);
  if (t == TILE_256) return go(Pw256{});
  if constexpr (kind_takes(KIND, TILE_256x64)) if (t == TILE_256x64) return go(Pw256x64{});
  if constexpr (kind_takes(KIND, TILE_64x256)) if (t == TILE_64x256) return go(Pw64x256{});
  return go(Pw128{});
}

// fp32 operands.  LAT / LBT: loader families <TILE, FMT, NT> of gemm_loaders.h.
template <LaunchKind KIND, template <int, class, int> class LAT, template <int, class, int> class LBT, class MKA, class MKB>
static int launch_gemm(MKA mka, MKB mkb, const EpiParams& ep, int M, int N, int K, int splitk, hipStream_t stream) {
  auto go = [&](auto rows, auto cols) {
    using LA = LAT<decltype(rows)::value, F32, NTHREADS>; using LB = LBT<decltype(cols)::value, F32, NTHREADS>;
    return launch_gemm<LA, LB, decltype(rows)::value / 64, decltype(cols)::value / 64>(mka(LoaderTag<LA>{}), mkb(LoaderTag<LB>{}), ep, M, N, K,
                                                                                      splitk, stream);
  };
  using I64 = std::integral_constant<int, 64>; using I128 = std::integral_constant<int, 128>; using I256 = std::integral_constant<int, 256>;
  const Tile t = pick_tile(KIND, M, N, K, splitk, false);
  if (t == TILE_256) return CXRK_ERR_UNSUPPORTED;   // the 256x256 kernel reads planes operands (use_wide256 never picks it here)
  if constexpr (kind_takes(KIND, TILE_256x64)) if (t == TILE_256x64) return go(I256{}, I64{});
  if constexpr (kind_takes(KIND, TILE_64x256)) if (t == TILE_64x256) return go(I64{}, I256{});
  return go(I128{}, I128{});
}

}  // namespace cxrk
