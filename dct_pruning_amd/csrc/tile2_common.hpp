// tile2_common.hpp - what the two 2-D radix-split families (tile2d.hip: 224 x 224, one map per round; tile2g.hip: edges
// 72 ... 160, G maps per round) share on top of split_roles.hpp: the role network on 2^L values held in registers, its
// rotation constants laid out for one 16-byte read per lane, the squared role weights and the register pin.
// What differs stays in each file: the block-parameter records (their LDS word order is baked into ds_read offsets), the
// schedules (T2Sched / G2Sched), T2Cfg / G2Cfg, the codelets, the passes and the bodies.
#pragma once
#include "split_roles.hpp"

namespace {

// rotation constants (c, s, sigma*c, sigma*s), sigma = (-1)^j of the pair index: [rot][p][4]
template <int L, int M>
struct Tile2RotTable {
  static constexpr int NROT = RolePlan<L>{}.nrot;
  float v[NROT > 0 ? NROT : 1][M][4] = {};
  constexpr Tile2RotTable() {
    constexpr RotTable<M, L> t{};
    for (int r = 0; r < NROT; ++r)
      for (int p = 0; p < M; ++p) {
        const float sg = RotTable<M, L>::sign0(r) * ((p & 1) ? -1.f : 1.f);
        v[r][p][0] = t.c[r][p];
        v[r][p][1] = t.s[r][p];
        v[r][p][2] = sg * t.c[r][p];
        v[r][p][3] = sg * t.s[r][p];
      }
  }
};
template <int L, int M>
__device__ const Tile2RotTable<L, M> kTile2Rot{};

// squared amplitude weights of role R's leaf outputs: output 0 / outputs > 0
template <int L, int M, int R>
constexpr void tile2_role_weights(float& w0, float& w1) {
  using Leaf = typename RoleLeaf<(M << L), L, R>::type;
  const double a = Leaf::wt(true), b = Leaf::wt(false);
  w0 = float(a * a);
  w1 = float(b * b);
}

// the value exists in a VGPR here: the compiler may not sink its computation past this point
__device__ __forceinline__ void tile2_pin(float& x) { asm volatile("" : "+v"(x)); }

// the L-level role network on 2^L values held in registers: y[slot], constants by lane
template <int L, int NROT>
__device__ __forceinline__ void tile2_network(float (&y)[1 << L], const float (&rc)[NROT > 0 ? NROT : 1][4]) {
  constexpr RolePlan<L> plan{};
  dcts::static_for<plan.NOPS>([&](auto i) DCTS_LAMBDA_INLINE {
    constexpr int o = decltype(i)::value;
    constexpr int a = plan.op_a[o], b = plan.op_b[o], r = plan.op_rot[o];
    const float ya = y[a], yb = y[b];
    if constexpr (r < 0) {
      y[a] = ya + yb;
      y[b] = ya - yb;
    } else {
      y[a] = ya * rc[r][0] + yb * rc[r][1];
      y[b] = yb * rc[r][2] - ya * rc[r][3];
    }
  });
}

}  // namespace
