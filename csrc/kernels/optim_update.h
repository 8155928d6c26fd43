// Scalar update expressions shared by the flat optimizers (optim.hip) and the layer-wise ones
// (optim_layerwise.hip): one copy of the momentum recurrence and of Adam's moments / denominator, so LARS is
// SGD's recurrence on a rescaled direction and LAMB is Adam's moments under a per-tensor trust ratio.
#pragma once

// SGD's momentum, dampening, Nesterov and first-step recurrence on the direction d; b is the momentum buffer
// element (read unless `first`, written when momentum != 0).  Returns the direction the parameter moves along.
__device__ __forceinline__ float sgd_momentum(float d, float& b, float momentum, float dampening, int nesterov,
                                              int first) {
    if (momentum != 0.f) {
        b = first ? d : momentum * b + (1.f - dampening) * d;
        d = nesterov ? d + momentum * b : b;
    }
    return d;
}

// Adam's first and second moments of the (already scaled) gradient gi; c1 = 1 - b1, c2 = 1 - b2.  The caller
// chooses how the complements are formed: 1.f - b2 in fp32 carries b2's rounding at 1 / (1 - b2) times its relative
// size (1.3e-5 at b2 = 0.999), a complement taken in double on the host and rounded once does not.
__device__ __forceinline__ void adam_moments(float gi, float& mi, float& vi, float b1, float b2, float c1, float c2) {
    mi = b1 * mi + c1 * gi;
    vi = b2 * vi + c2 * gi * gi;
}

// sqrt(v / bc2) + eps with rbc2 = rsqrt(bc2): eps is added to the bias-corrected root (torch.optim.Adam's order).
__device__ __forceinline__ float adam_denom(float vi, float rbc2, float eps) { return sqrtf(vi) * rbc2 + eps; }
