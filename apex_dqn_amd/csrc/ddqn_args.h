// Arguments of ddqn_head_kernel (csrc/ddqn_head.hip, which says what hp and pk do; ops/_lib.py DdqnArgs is the
// mirror).  A header of its own: csrc/sumtree.hip apex_abi_struct_sizes reports its size, and the other head files
// do not need the conv2 pack job.
#pragma once
#include "conv2_wfrag.h"
#include "head_common.h"

struct DdqnArgs {
  HeadIO io;            // Hon [2B], Htg [B]; dhead [B][1 + A]
  int huber;
  float kappa;
  HeadPart hp;
  C2dPackJob pk;
};
static_assert(std::is_standard_layout_v<DdqnArgs> && std::is_trivially_copyable_v<DdqnArgs>);
