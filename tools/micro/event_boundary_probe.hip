// Stand-alone probe: what does a cross-stream fork / join cost ON the forking stream's dependent chain
// (MI355X, ROCm 7.2), and does a cheaper event flag still publish the data?
//
// Why: the training step's caller's stream shows a 6-8 us hole at every hipEventRecord / hipStreamWaitEvent
// that unet.hip issues on it (profiles/r04_step_timeline.txt), against ~1.5 us for a plain dependent boundary.
//
// A dependent chain of LEN kernels runs on one stream S.  Two chains:
//   T  every kernel is a trivial 256-workgroup kernel (writes 256 KB)
//   D  a 64 MB streaming-store kernel and the trivial kernel alternate: the predecessor of every second
//      boundary leaves a full L2 of dirty lines, as a convolution does (Dnt: the same with nontemporal stores)
// Between consecutive kernels, per variant:
//   none  nothing
//   rec   hipEventRecord(e, S) that a LOW-priority stream B waits for; B then verifies what S's kernel wrote
//   wait  hipStreamWaitEvent(S, f), f recorded on B behind a kernel of B; S's next kernel verifies what B wrote
//   both  rec + wait (the wait on B's event of two boundaries earlier: no round trip, like ev_dy + ev_w)
// with the events created by hipEventDisableTiming alone (what the plan does), | hipEventReleaseToDevice,
// and | hipEventDisableSystemFence.  The host enqueues the whole chain while a ~4 ms spin kernel holds S, so the
// time between the spin's end and the chain's end is the GPU's, not the enqueue rate's.  Printed: the chain's
// median time over REPS repetitions and (median - median of `none`) / boundaries, in us.
//
// Correctness: producer and consumer are on different streams; every consumer reads 64 KB (16 Ki words, each
// compared with the value its producer must have written) and re-reads the first 4 KB; buffers are rewritten
// with new values every repetition, so a line left over in a cache shows as a stale word.  `stale` must be 0.
//
//   hipcc --offload-arch=gfx950 -O2 -o event_boundary_probe event_boundary_probe.hip && ./event_boundary_probe
// One process, run once.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#define CK(x)                                                                        \
  do {                                                                               \
    hipError_t e__ = (x);                                                            \
    if (e__ != hipSuccess) {                                                         \
      printf("%s -> %s (line %d)\n", #x, hipGetErrorString(e__), __LINE__);          \
      fflush(stdout);                                                                \
      return 2;                                                                      \
    }                                                                                \
  } while (0)

constexpr int LEN = 32;                   // kernels per chain
constexpr int REPS = 7;
constexpr uint32_t SMALL_WORDS = 1 << 16; // 256 workgroups x 256 threads, one word each
constexpr uint32_t CHECK_WORDS = 1 << 14; // 64 KB verified per hand-off
constexpr uint32_t REREAD_WORDS = 1 << 10;
constexpr size_t BIG_WORDS = (size_t)16 << 20;  // 64 MB

// verify CHECK_WORDS words of `c` (written as tag + index) and re-read its first 4 KB
__device__ void verify(const uint32_t* c, uint32_t off, uint32_t tag, uint32_t i, unsigned* stale) {
  if (!c || i >= CHECK_WORDS) return;
  const volatile uint32_t* v = c;
  unsigned bad = v[off + i] != tag + off + i;
  const uint32_t j = i & (REREAD_WORDS - 1);
  bad += v[off + j] != tag + off + j;
  if (bad) atomicAdd(stale, bad);
}

// the chain's trivial kernel, also B's kernel: verify `c`, then write n words of `own`
__global__ void small_kernel(uint32_t* own, uint32_t n, uint32_t tag, const uint32_t* c, uint32_t off, uint32_t ctag,
                             unsigned* stale) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  verify(c, off, ctag, i, stale);
  if (i < n) own[i] = tag + i;
}

// 64 MB of 16-byte stores, word w = tag + w
__global__ void big_kernel(uint4* p, uint32_t n4, uint32_t tag, int nt) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += gridDim.x * blockDim.x) {
    const uint32_t w = tag + 4 * i;
    if (nt) {
      __builtin_nontemporal_store(w, &p[i].x);
      __builtin_nontemporal_store(w + 1, &p[i].y);
      __builtin_nontemporal_store(w + 2, &p[i].z);
      __builtin_nontemporal_store(w + 3, &p[i].w);
    } else {
      p[i] = make_uint4(w, w + 1, w + 2, w + 3);
    }
  }
}

__global__ void spin_kernel(long long ticks) {   // wall_clock64: 100 MHz
  const long long t0 = wall_clock64();
  for (int k = 0; k < (1 << 20) && wall_clock64() - t0 < ticks; ++k) __builtin_amdgcn_s_sleep(8);
}

enum Op { NONE, REC, WAIT, BOTH };
static const char* op_name[] = {"none", "rec", "wait", "both"};

int main() {
  hipStream_t S, B;
  int lo = 0, hi = 0;
  CK(hipDeviceGetStreamPriorityRange(&lo, &hi));
  CK(hipStreamCreateWithFlags(&S, hipStreamNonBlocking));
  CK(hipStreamCreateWithPriority(&B, hipStreamNonBlocking, lo));
  uint32_t *sm[LEN], *ym[LEN], *big[LEN / 2];
  for (int j = 0; j < LEN; ++j) {
    CK(hipMalloc(&sm[j], SMALL_WORDS * 4));
    CK(hipMalloc(&ym[j], CHECK_WORDS * 4));
    CK(hipMemset(sm[j], 0, SMALL_WORDS * 4));
    CK(hipMemset(ym[j], 0, CHECK_WORDS * 4));
  }
  for (int j = 0; j < LEN / 2; ++j) {
    CK(hipMalloc(&big[j], BIG_WORDS * 4));
    CK(hipMemset(big[j], 0, BIG_WORDS * 4));
  }
  unsigned* stale;
  CK(hipMalloc(&stale, 4));
  hipEvent_t t0, t1;
  CK(hipEventCreate(&t0));
  CK(hipEventCreate(&t1));
  CK(hipDeviceSynchronize());

  struct FlagSet { const char* name; unsigned flags; };
  const FlagSet sets[] = {{"DisableTiming", hipEventDisableTiming},
                          {"DisableTiming|ReleaseToDevice", hipEventDisableTiming | hipEventReleaseToDevice},
                          {"DisableTiming|DisableSystemFence", hipEventDisableTiming | hipEventDisableSystemFence}};
  uint32_t serial = 1;   // every kernel of the run writes a tag of its own
  printf("chain of %d kernels, %d boundaries, %d repetitions; us\n", LEN, LEN - 1, REPS);
  printf("%-4s %-5s %-34s %10s %10s %12s %6s\n", "kind", "op", "event flags", "median", "min", "per boundary", "stale");

  for (int kind = 0; kind < 3; ++kind) {   // 0: T, 1: D, 2: Dnt
    const char* kname = kind == 0 ? "T" : kind == 1 ? "D" : "Dnt";
    float base = 0.f;
    for (int fs = 0; fs < 3; ++fs) {
      hipEvent_t e[LEN], f[LEN];
      bool ok = true;
      for (int j = 0; j < LEN && ok; ++j)
        ok = hipEventCreateWithFlags(&e[j], sets[fs].flags) == hipSuccess &&
             hipEventCreateWithFlags(&f[j], sets[fs].flags) == hipSuccess;
      if (!ok) {
        (void)hipGetLastError();
        printf("%-4s %-5s %-34s not accepted by hipEventCreateWithFlags\n", kname, "-", sets[fs].name);
        continue;
      }
      for (int op = fs == 0 ? NONE : REC; op <= (kind == 2 ? NONE : BOTH); ++op) {
        CK(hipMemsetAsync(stale, 0, 4, S));
        CK(hipDeviceSynchronize());
        std::vector<float> ms;
        for (int r = 0; r < REPS; ++r) {
          spin_kernel<<<1, 64, 0, S>>>(400000);   // 4 ms
          CK(hipEventRecord(t0, S));
          // what S's kernel j-1 wrote, for whoever verifies it
          const uint32_t* prev = nullptr;
          uint32_t prev_off = 0, prev_tag = 0;
          uint32_t ytag[LEN] = {};
          for (int j = 0; j < LEN; ++j) {
            if (j > 0) {
              if (op == REC || op == BOTH) {
                CK(hipEventRecord(e[j], S));
                CK(hipStreamWaitEvent(B, e[j], 0));
              }
              if (op != NONE) {   // B: verify S's last kernel (rec, both), write y[j], record f[j]
                ytag[j] = serial += 0x10001;
                const bool chk = op != WAIT;
                small_kernel<<<CHECK_WORDS / 256, 256, 0, B>>>(ym[j], CHECK_WORDS, ytag[j], chk ? prev : nullptr, prev_off,
                                                               prev_tag, stale);
                CK(hipEventRecord(f[j], B));
              }
              const int jw = op == WAIT ? j : j - 2;   // both: B's event of two boundaries earlier
              if ((op == WAIT || op == BOTH) && jw > 0) CK(hipStreamWaitEvent(S, f[jw], 0));
            }
            const uint32_t tag = serial += 0x10001;
            if (kind > 0 && (j & 1) == 0) {
              big_kernel<<<2048, 256, 0, S>>>(reinterpret_cast<uint4*>(big[j / 2]), (uint32_t)(BIG_WORDS / 4), tag, kind == 2);
              prev = big[j / 2]; prev_off = (uint32_t)(BIG_WORDS - CHECK_WORDS); prev_tag = tag;   // the last lines written
            } else {
              // verifies B's y (wait, both) or the chain's own previous kernel (none, rec): the same work in every variant
              const uint32_t* c = prev;
              uint32_t off = prev_off, ctag = prev_tag;
              const int jw = op == WAIT ? j : j - 2;
              if (op == WAIT || op == BOTH) {
                c = jw > 0 ? ym[jw] : nullptr; off = 0; ctag = jw > 0 ? ytag[jw] : 0;
              }
              small_kernel<<<SMALL_WORDS / 256, 256, 0, S>>>(sm[j], SMALL_WORDS, tag, c, off, ctag, stale);
              prev = sm[j]; prev_off = 0; prev_tag = tag;
            }
          }
          CK(hipEventRecord(t1, S));
          CK(hipGetLastError());
          CK(hipDeviceSynchronize());
          float t = 0.f;
          CK(hipEventElapsedTime(&t, t0, t1));
          ms.push_back(t * 1e3f);
        }
        unsigned h = 0;
        CK(hipMemcpy(&h, stale, 4, hipMemcpyDeviceToHost));
        std::sort(ms.begin(), ms.end());
        const float med = ms[REPS / 2];
        if (op == NONE) base = med;
        printf("%-4s %-5s %-34s %10.1f %10.1f %12.2f %6u\n", kname, op_name[op], op == NONE ? "-" : sets[fs].name, med,
               ms[0], (med - base) / (LEN - 1), h);
        fflush(stdout);
      }
      for (int j = 0; j < LEN; ++j) { (void)hipEventDestroy(e[j]); (void)hipEventDestroy(f[j]); }
    }
  }
  return 0;
}
