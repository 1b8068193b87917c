// encoder_general.hpp — the layered split-f16 MFMA encoder for every frame shape the fused 64x64x3 kernel
// (encoder.hip) does not cover: 224x224x3 (the reference's RENDER_HEIGHT/WIDTH), 6-channel multi_view frames, ...
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "../../include/srlhip.h"
#include "encoder_pack.hpp"

namespace srlenc {

struct General;                  // device buffers + geometry of one encoder handle

// weights in torch layout with the BatchNorms folded (see srlhip.h); fc_w is [state_dim][64 * Wp3 * Hp3] in torch's
// flatten order of the TRANSPOSED frame (channel, frame column, frame row).  *out is set as soon as the handle exists: on an error the
// caller destroys it.
int general_create(int device_id, const Geometry &g, int state_dim, const float *conv1_w, const float *conv1_b, const float *conv2_w,
                   const float *conv2_b, const float *conv3_w, const float *conv3_b, const float *fc_w, const float *fc_b,
                   General **out, std::string &err);
int general_forward(General *g, const uint8_t *images_dev, int n, float *states_dev, hipStream_t stream, std::string &err);
int *general_status(General *g);
void general_destroy(General *g);

// The HIP check of the encoder's two translation units: a failed call leaves "<call as written>: <HIP's error string>" in err and
// returns SRLHIP_EHIP from the calling function, which leaves the cleaning up to its caller or to a destructor.
inline bool hip_failed(hipError_t rc, const char *call, std::string &err) {
    if (rc != hipSuccess) err = std::string(call) + ": " + hipGetErrorString(rc);
    return rc != hipSuccess;
}
#define ENC_HIP(err, expr)                                                        \
    do {                                                                          \
        if (::srlenc::hip_failed((expr), #expr, (err))) return SRLHIP_EHIP;       \
    } while (0)

}  // namespace srlenc
