// k_pg.cuh — group-wise (per-group) quantization: the view shared by the kernels of
// k_pg.hip and the host loops of k_host.hip.
//
// A [rows, rowlen] tensor (axis 0 rows, as K3) is cut into groups of `group` consecutive
// elements of a row: ngr = ceil(rowlen / group) groups per row, group j of row r covering
// elements [j*group, min((j+1)*group, rowlen)) -- groups restart at every row and the last
// one of a row may be short.  The qparams of group (r, j) live at index r*ngr + j.
#pragma once
#include <stdint.h>

namespace vsiq {

inline bool pg_group_ok(int64_t group) { return group == 32 || group == 64 || group == 128 || group == 256; }
inline int64_t pg_groups_per_row(int64_t rowlen, int64_t group) { return (rowlen + group - 1) / group; }

}  // namespace vsiq
