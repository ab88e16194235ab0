// eval.hip — evaluation of a batch of scores against its labels (the reference's `test`,
// src/train/utils.jl:31-46, plus log loss and the ranking AUC needs), folded into device-resident
// integer counters: one launch per batch, no host synchronisation, hipGraph-capturable.
//   eval_accumulate_kernel  prob (bce_head_kernel's sigmoid), rintf(prob) == label, the bce_loss
//                           term (train.jl:33-41) and a histogram of prob's upper float bits per class
// State words (include/dlrm_hip.h has the table): 0 total, 1 correct, 2 positives, 3 negatives,
// 4 batches, 5 loss_sum (double bits), 6 the last call's mean loss (float bits), 7 zero, then
// hist[2][kEvalBins].  Integer atomics only, and the loss is reduced in bce_head_kernel's fixed order:
// every word is reproducible.
#include "common.hpp"

namespace dlrm {

constexpr int kEvalThreads = 1024;
constexpr unsigned kOneBits = 0x3F800000u;  // float bits of 1.0f: positive floats order as their bits do
static_assert(kEvalBins == (int)(kOneBits >> kEvalShift) + 1, "one bin per truncated key in [0, 1]");

// One workgroup looping over the batch, like bce_head_kernel (the pass is bound by the MLP GEMMs).
template <bool IS_PROB>
__global__ void __launch_bounds__(kEvalThreads)
eval_accumulate_kernel(int B, const float* __restrict__ s, int64_t s_ld, const float* __restrict__ y,
                       float* __restrict__ prob, unsigned long long* __restrict__ state) {
    constexpr int NW = kEvalThreads / kWave;
    __shared__ float sl[NW];
    __shared__ unsigned sc[NW], sp[NW], sn[NW];
    unsigned long long* hist = state + kEvalHeader;
    const float inv = 1.0f / (float)B;
    float l = 0.0f;
    unsigned correct = 0, pos = 0, neg = 0;
    for (int i = threadIdx.x; i < B; i += kEvalThreads) {
        const float zi = s[(int64_t)i * s_ld], yi = y[i];
        float p;
        if (IS_PROB)
            p = zi;
        else
            p = 1.0f / (1.0f + __expf(-zi));  // bce_head_kernel's sigmoid: the bits training sees
        l += -yi * fmaxf(__logf(p), -100.0f) + (yi - 1.0f) * fmaxf(__logf(1.0f - p), -100.0f);
        if (prob) prob[i] = p;
        // round.(predictions) .== labels: ties to even (0.5 predicts 0); a soft label or a NaN is never equal
        correct += rintf(p) == yi ? 1u : 0u;
        // the key: float bits of p clamped to [0, 1] (fmaxf drops a NaN: bin 0); the integer clamp keeps the bin
        // in range whatever bits arrive (-0.0f among them)
        const float pc = fminf(fmaxf(p, 0.0f), 1.0f);
        const int bits = min(max((int)__float_as_uint(pc), 0), (int)kOneBits);
        const int k = bits >> kEvalShift;
        if (yi == 1.0f) {
            atomicAdd(hist + kEvalBins + k, 1ull);
            ++pos;
        } else if (yi == 0.0f) {
            atomicAdd(hist + k, 1ull);
            ++neg;
        }
    }
    // wave sums (fixed butterfly order), then the 16 wave partials in wave order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        l += __shfl_xor(l, o);
        correct += __shfl_xor(correct, o);
        pos += __shfl_xor(pos, o);
        neg += __shfl_xor(neg, o);
    }
    const int w = threadIdx.x / kWave;
    if ((threadIdx.x & (kWave - 1)) == 0) {
        sl[w] = l;
        sc[w] = correct;
        sp[w] = pos;
        sn[w] = neg;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float L = 0.0f;
        unsigned C = 0, P = 0, N = 0;
        for (int k = 0; k < NW; ++k) {
            L += sl[k];
            C += sc[k];
            P += sp[k];
            N += sn[k];
        }
        atomicAdd(state + 0, (unsigned long long)B);
        atomicAdd(state + 1, (unsigned long long)C);
        atomicAdd(state + 2, (unsigned long long)P);
        atomicAdd(state + 3, (unsigned long long)N);
        atomicAdd(state + 4, 1ull);
        // calls on one stream serialise: a plain read-modify-write, the sum in call order
        state[5] = (unsigned long long)__double_as_longlong(__longlong_as_double((long long)state[5]) + (double)L);
        state[6] = (unsigned long long)__float_as_uint(L * inv);
    }
}

int launch_eval_accumulate(dlrm_ctx* ctx, unsigned long long* state, int B, const float* scores, int64_t scores_ld,
                           bool is_prob, const float* labels, float* prob) {
    auto* kern = is_prob ? eval_accumulate_kernel<true> : eval_accumulate_kernel<false>;
    hipLaunchKernelGGL(kern, dim3(1), dim3(kEvalThreads), 0, ctx_stream(ctx), B, scores, scores_ld, labels, prob,
                       state);
    return ctx_hip(ctx, hipGetLastError(), "eval_accumulate launch");
}

}  // namespace dlrm
