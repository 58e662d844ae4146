// bz_ownership.h -- ownership targets: from a finished game's final board in absolute colours (fin_x = X's
// stones, X = the side that moves with to_move = +1; fin_o = O's) to the board a recorded row is trained on, in that row's
// side-to-move frame.  __host__ __device__ so that bz_ownership_row (host) is the code k_pack_own runs.
#pragma once
#include "bz_math.h"

namespace bz {

// the row's target boards: t_own = the cells the row's mover owns at the end, t_opp = the other side's.  The target of cell
// i is bit_i(t_own) - bit_i(t_opp) in {+1, 0, -1}: an empty cell gives 0, and so does a cell outside the board.
BZ_HD void ownership_row(u64 fin_x, u64 fin_o, int mover, u64* t_own, u64* t_opp) {
    const bool x = mover == 1;
    *t_own = x ? fin_x : fin_o;
    *t_opp = x ? fin_o : fin_x;
}

}  // namespace bz
