// optim.hip.h -- TensorFlow's Adam and FTRL updates of one variable element, shared by the inner-product family
// (ip_step_kernels.hip.h, a part of the unit ipnn_api.hip) and factorisation-machine pre-training (fm_kernels.hip.h, a part of
// the unit fm_api.hip).  Internal, not installed.
#pragma once
#include <hip/hip_runtime.h>

namespace fnn {

// tf.train.AdamOptimizer (python/tf_util.py:17-20): lr_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t) of this step, computed on
// the host; state = (m, v).
__device__ inline float adam_step(float w, float g, float& m, float& v, float lr_t, float b1, float b2, float eps) {
    m = b1 * m + (1.0f - b1) * g;
    v = b2 * v + (1.0f - b2) * g * g;
    return w - lr_t * m / (sqrtf(v) + eps);
}

// TensorFlow's FtrlOptimizer(learning_rate) as python/tf_util.py:21-24 builds it (learning_rate_power -0.5, initial
// accumulator 0.1, l1 = l2 = 0; the ApplyFtrl kernel): state = (accum, linear).  A variable with a zero gradient keeps its
// accumulator and linear term, and is RE-DERIVED from them: w = -linear lr / sqrt(accum) -- with a dense table gradient,
// rows no example has touched yet drop to 0 at the first step, as they do in the reference.
__device__ inline float ftrl_step(float w, float g, float& accum, float& linear, float lr) {
    const float na = accum + g * g, sa = sqrtf(na);
    linear += g - g * g / (sa + sqrtf(accum)) / lr * w;         // sqrt(na) - sqrt(accum), written without the cancellation
    accum = na;
    return linear != 0.f ? -linear / (sa / lr) : 0.f;
}

}  // namespace fnn
