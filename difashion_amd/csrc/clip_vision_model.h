// The context of the CLIP image encoder (dfh_clipv, made by dfh_clipv_create in clip_vision.hip): config, parameter table and the fp32
// workspace layout.  Shared by the fp32 walk (clip_vision.hip) and the 16-bit walk (clip_vision_half.hip).
#pragma once
#include "../../include/difashion_hip.h"
#include "clip_tower.h"

struct dfh_clipv : dfh::ParamList {
  dfh_clipv_config cfg{};
  int cls = 0, patch = 0, pos = 0, prew = 0, preb = 0, postw = 0, postb = 0, proj = 0;
  std::vector<dfh::ClipLayer> layers;
  int grid = 0, T = 0, Kp = 0;     // patches per side, tokens, C * p * p
  // the q k v region doubles as the im2col rows of the patch conv (the attention region as its output); tail: the pooled row of every image
  dfh::ClipWorkspace workspace(void* base, int batch) const {
    const size_t D = cfg.hidden_size;
    return dfh::ClipWorkspace(base, (size_t)batch * T, D, cfg.intermediate_size, 3 * D > (size_t)Kp ? 3 * D : (size_t)Kp, (size_t)batch * D);
  }
};
