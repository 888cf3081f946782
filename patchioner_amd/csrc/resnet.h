// RegionCLIP's ModifiedResNet tower (vit_arch 3): the interface between api.cpp and resnet_api.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include <functional>
#include <string>

#include "../../include/patchioner_hip.h"

namespace pio {

struct RnNet;
// the weight under `key`, which must hold `numel` floats: 0 and *data set, or a pio_status with the message set
typedef std::function<int(const std::string& key, int64_t numel, const float** data)> RnGet;
// packs the tower's weights (keys "rn.*", weights.regionclip_to_engine) and sizes its workspaces for cfg.max_batch images
int rn_build(const pio_config& cfg, const RnGet& get, RnNet** out);
void rn_destroy(RnNet* r);
size_t rn_workspace_bytes(const RnNet* r);
// imgs [B][3][crop][crop] fp32 -> tokens [B][1 + (crop/32)^2][Dout] fp32, L2-normalised rows; enqueue only
int rn_forward(RnNet* r, const float* imgs, int B, float* tokens, hipStream_t s);

}  // namespace pio
