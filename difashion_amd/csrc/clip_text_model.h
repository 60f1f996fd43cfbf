// The context of the CLIP text encoder (dfh_clip, made by dfh_clip_create in clip.hip): config, parameter table and the fp32 workspace
// layout.  Shared by the fp32 walk (clip.hip) and the 16-bit walk (clip_text_half.hip).
#pragma once
#include "../../include/difashion_hip.h"
#include "clip_tower.h"

struct dfh_clip : dfh::ParamList {
  dfh_clip_config cfg{};
  int tok = 0, pos = 0, fw = 0, fb = 0;
  std::vector<dfh::ClipLayer> layers;
  dfh::ClipWorkspace workspace(void* base, int batch, int T) const {
    return dfh::ClipWorkspace(base, (size_t)batch * T, cfg.hidden_size, cfg.intermediate_size, 3 * (size_t)cfg.hidden_size, 0);
  }
};
