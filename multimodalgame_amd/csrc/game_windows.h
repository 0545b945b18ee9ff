// game_windows.h -- index arithmetic of k_game_fast's baseline roles (kernels_game.h: game_baseline_role), host-callable so that
// tests/test_game_windows_cpu.py can check it exhaustively against `/` and `%` (mmg_game_window_split / _counts, mmg.hip).
//
// The live (step, sample) rows of a minibatch are cut into windows of 16; window w belongs to slot w % nslots and is that slot's
// (w / nslots)-th window.  nslots is a run-time value: hipcc expands every `/` and `%` by it into ~35 dependent instructions
// around v_rcp_iflag_f32, on the one wave that builds the list while the statistics chain waits for it.  Here the reciprocal is
// formed once (while the role waits for the forward passes anyway) and a quotient is a multiply and a shift.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

namespace mmg {

// floor(n / nslots) = (n * mul) >> 19 with mul = floor(2^19 / nslots) + 1, exact while n * (mul * nslots - 2^19) < 2^19: the
// excess is at most nslots <= 64 and n < 65 * 64, so n * excess < 2^19; n * mul < 2^32 (nslots = 1: 64 * (2^19 + 1)).
struct GameWinDiv { uint32_t mul; int nslots; };
constexpr int GAME_WIN_SHIFT = 19, GAME_WIN_MAX_SLOTS = 64, GAME_WIN_PER_SLOT = 64;

__host__ __device__ inline GameWinDiv game_win_div(int nslots) { return GameWinDiv{(1u << GAME_WIN_SHIFT) / (uint32_t)nslots + 1u, nslots}; }
// n / nslots for 0 <= n < 65 * nslots, nslots <= 64
__host__ __device__ inline int game_win_quot(const GameWinDiv& d, int n) { return (int)(((uint32_t)n * d.mul) >> GAME_WIN_SHIFT); }
// window w of the minibatch: its index among its slot's windows (kw = w / nslots) and its slot (w % nslots)
__host__ __device__ inline void game_win_split(const GameWinDiv& d, int w, int& kw, int& slot) { kw = game_win_quot(d, w); slot = w - kw * d.nslots; }
// windows of `slot` when the minibatch has nw: slot, slot + nslots, ... below nw
__host__ __device__ inline int game_win_count(const GameWinDiv& d, int nw, int slot) { return nw > slot ? game_win_quot(d, nw - slot + d.nslots - 1) : 0; }

// An entry of a role's row list: the live row t * B + b with its sample b (B <= 64) in the low six bits, so that the consumers of
// the list -- the basehx pairs of the sample -- need no `% B`; -1 = no row (every field of it reads as "none": row -1).
__host__ __device__ inline int game_row_pack(int t, int B, int b) { return ((t * B + b) << 6) | b; }
__host__ __device__ inline int game_row_id(int e) { return e >> 6; }               // (arithmetic shift: -1 stays -1)
__host__ __device__ inline int game_row_sample(int e) { return e & 63; }

}  // namespace mmg
