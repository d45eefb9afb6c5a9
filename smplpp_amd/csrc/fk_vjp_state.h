// The per-model state the FK backward (fk_vjp.hip) and the FK forward mode (fk_jvp.hip) share: the operand image BT, the workspace in
// which either recomputes the rest shape, and each call's own buffers.  Created by the first backward or forward-mode call on a model.
#pragma once

#include "common.h"

namespace smplpp_hip
{
constexpr int VJ_KN = 224; // columns of the operand image (k < 217 live)

struct VjpState
{
  DevPtr<float> BT;     // operand image [VGn*32*3][224] fp32, row (v, x) = [P[v][x][0..207) | S[v][x][0..10) | 0 x 7] (fk_vjp.hip)
  Workspace fws;        // the forward's workspace while smplpp_fk_vjp recomputes `rest` (smplpp_fk's own stays untouched)
  DevPtr<int> range_word; // where that recomputation reports an fp16x2 range miss (not smplpp_fk's words)
  DevBuf Gp, joints, rot, slab;
  DevBuf rest;          // the rest shape recomputed when the caller passes none
  DevBuf jcoef, jrec;   // forward mode: the coefficient rows and the per-column transforms of jvp_chain_kernel (fk_jvp.hip)
};

// the state of a model (created on its first use)
int fk_vjp_state(smplpp_model * m);
// the operand image, built on its first use on the model (on `st`)
int fk_vjp_image(smplpp_model * m, hipStream_t st, const float ** BT);
// the rest shape [n][V][3] of (beta, pose) recomputed with the model's form into the state's own workspace: smplpp_fk's workspace,
// range words and profiling record stay as they were.  rot_in: pose = rot [n][24][9] with `trans`, else theta [n][25][3]
int fk_vjp_rest(smplpp_model * m, int64_t n, const float * beta, const float * pose, const float * trans, bool rot_in, hipStream_t st,
                const float ** rest);
} // namespace smplpp_hip
