// Host-side argument checks of the four head-dim-32 attention entry points under AddressSanitizer / UBSan, as a stand-alone program: every call
// below must be REJECTED by a check in front of any HIP call (so small integers stand in for the device pointers, and no GPU is needed), with a
// message that names the entry point.  Only the host code is instrumented; nothing here ever launches a kernel.
//
//   cd cl-drd_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Wno-unused-value -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-omit-frame-pointer ../../tools/micro/hd32_argcheck.hip attention_hd32.hip encoder_f32.hip capi.hip -o /tmp/hd32_argcheck
//   /tmp/hd32_argcheck          # prints "hd32_argcheck: N calls rejected" and exits 0
#include <cstdio>
#include <cstring>

#include "../../include/cldrd_hip.h"

static int failures = 0, calls = 0;

static void rejected(const char* op, int rc) {
    ++calls;
    const char* msg = cldrd_last_error();
    const size_t n = strlen(op);
    if (rc == 0 || strncmp(msg, op, n) != 0 || msg[n] != ':') {
        fprintf(stderr, "%s: rc %d, message '%s'\n", op, rc, msg);
        ++failures;
    }
    cldrd_set_tuning(nullptr, 0);       // leaves "set_tuning: null key" behind: the next message is the next call's own
}

int main() {
    void* const P = (void*)64;
    const long long* const M = (const long long*)64;
    const int* const I = (const int*)64;
    const float* const F = (const float*)64;
    float* const O = (float*)64;
    const int nseq = 4, L = 32, H = 2;
    const char* fwd = "attention_fwd_hd32";
    rejected(fwd, cldrd_attention_fwd_hd32(P, M, I, nullptr, 0, 0, P, nseq, L, H, 0, nullptr, nullptr));          // mask together with cu_rows
    rejected(fwd, cldrd_attention_fwd_hd32(P, nullptr, nullptr, nullptr, 0, 0, P, nseq, 257, H, 0, nullptr, nullptr));
    rejected(fwd, cldrd_attention_fwd_hd32(P, nullptr, nullptr, nullptr, 0, 0, P, nseq, 0, H, 0, nullptr, nullptr));
    rejected(fwd, cldrd_attention_fwd_hd32(P, nullptr, nullptr, nullptr, 0, 0, P, nseq, L, 3, 0, nullptr, nullptr));        // odd H
    rejected(fwd, cldrd_attention_fwd_hd32(P, nullptr, nullptr, nullptr, 0, 0, P, nseq, L, H, 5, nullptr, nullptr));        // fmt
    rejected(fwd, cldrd_attention_fwd_hd32(P, nullptr, nullptr, nullptr, 0, 0, nullptr, nseq, L, H, 0, nullptr, nullptr));  // no output
    rejected(fwd, cldrd_attention_fwd_hd32(P, nullptr, nullptr, I, 2, L, P, nseq, L, H, 0, nullptr, nullptr));              // seq_list without cu_rows
    rejected(fwd, cldrd_attention_fwd_hd32(P, nullptr, I, I, nseq + 1, L, P, nseq, L, H, 0, nullptr, nullptr));
    rejected(fwd, cldrd_attention_fwd_hd32(P, nullptr, I, I, 2, L + 1, P, nseq, L, H, 0, nullptr, nullptr));
    rejected(fwd, cldrd_attention_fwd_hd32(P, nullptr, nullptr, nullptr, 0, 0, P, nseq, L, H, 1, P, nullptr));               // the fp16 pass writes ctx only
    const char* cls = "attention_cls_fwd_hd32";
    rejected(cls, cldrd_attention_cls_fwd_hd32(P, P, M, I, P, nseq, L, H, 0, nullptr, nullptr));
    rejected(cls, cldrd_attention_cls_fwd_hd32(P, P, nullptr, nullptr, P, nseq, 257, H, 0, nullptr, nullptr));
    rejected(cls, cldrd_attention_cls_fwd_hd32(P, P, nullptr, nullptr, P, nseq, L, 5, 0, nullptr, nullptr));
    rejected(cls, cldrd_attention_cls_fwd_hd32(P, P, nullptr, nullptr, P, nseq, L, H, 5, nullptr, nullptr));
    rejected(cls, cldrd_attention_cls_fwd_hd32(P, P, nullptr, nullptr, nullptr, nseq, L, H, 0, nullptr, nullptr));
    rejected(cls, cldrd_attention_cls_fwd_hd32(nullptr, P, nullptr, nullptr, P, nseq, L, H, 0, nullptr, nullptr));
    const char* f32 = "attention_fwd_f32_hd32";
    rejected(f32, cldrd_attention_fwd_f32_hd32(F, M, I, O, nseq, L, H, nullptr));
    rejected(f32, cldrd_attention_fwd_f32_hd32(F, nullptr, nullptr, O, nseq, 257, H, nullptr));
    rejected(f32, cldrd_attention_fwd_f32_hd32(F, nullptr, nullptr, nullptr, nseq, L, H, nullptr));
    rejected(f32, cldrd_attention_fwd_f32_hd32(nullptr, nullptr, nullptr, O, nseq, L, H, nullptr));
    rejected(f32, cldrd_attention_fwd_f32_hd32((const float*)68, nullptr, nullptr, O, nseq, L, H, nullptr));               // not 16-byte aligned
    rejected(f32, cldrd_attention_fwd_f32_hd32(F, nullptr, nullptr, O, 0x7FFFFFFF, L, H, nullptr));                         // batch too large
    const char* c32 = "attention_cls_fwd_f32_hd32";
    rejected(c32, cldrd_attention_cls_fwd_f32_hd32(F, H * 32, F, M, I, O, nseq, L, H, nullptr));
    rejected(c32, cldrd_attention_cls_fwd_f32_hd32(F, H * 32, F, nullptr, nullptr, O, nseq, 257, H, nullptr));
    rejected(c32, cldrd_attention_cls_fwd_f32_hd32(F, H * 32 - 4, F, nullptr, nullptr, O, nseq, L, H, nullptr));            // pitch shorter than a row
    rejected(c32, cldrd_attention_cls_fwd_f32_hd32(F, H * 32 + 2, F, nullptr, nullptr, O, nseq, L, H, nullptr));
    rejected(c32, cldrd_attention_cls_fwd_f32_hd32(F, H * 32, F, nullptr, nullptr, nullptr, nseq, L, H, nullptr));
    printf("hd32_argcheck: %d calls rejected, %d failures\n", calls - failures, failures);
    return failures != 0;
}
