// Launch log of the flagship executor, on the CPU: this program defines the HIP runtime entry points libadt_hip.so imports (its own symbols come
// first in the lookup order, so nothing is preloaded and no GPU is touched), loads the given library, runs the flagship case list and logs every
// launch: kernel name, grid, block, dynamic LDS, every byte of every kernel argument, the stream, every event record / wait, every
// hipFuncSetAttribute and every return code with its adt_last_error text.  A host-only change of the executor must leave the log as it was:
// tools/launch_log.py runs it on a build of the parent commit against a build of the change.
//
//   launch_log <libadt_hip.so> <argsizes.txt> <poison byte>                           one line per configuration: launches and two digests
//   launch_log <libadt_hip.so> <argsizes.txt> <poison byte> <prec> <H> <L> <layers> <B>  that configuration's log itself
//   launch_log <libadt_hip.so> <argsizes.txt> <poison byte> <other libadt_hip.so>       both libraries in one process, compared record by record
//
// The first digest of a configuration covers everything but the argument bytes (kernels, grids, blocks, LDS, argument sizes, streams, events,
// attributes, return codes, error texts), the second the argument bytes too.  argsizes.txt (written by the driver from the code objects'
// metadata): "<kernel symbol> <n> <size of argument 0> ...".  Device pointers are fixed made-up values; what the host layer dereferences (cfg,
// lambdas2, the layer pointer structs) lives in an arena mapped at a fixed address, so that no address in the log depends on the process.
// Argument bytes the host code never writes -- struct padding, the unused tail of a fixed-size array -- hold whatever the stack held, which
// differs from build to build: the comparison mode knows the padding of the argument structs the case list reaches (PADDING) and the two counted
// arrays (COUNTED); a differing byte anywhere else makes the record unequal, like any other difference.  It also lists every offset that differed.  The stack is filled with the poison byte in
// front of every call.
#include <dlfcn.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>

#include <map>
#include <string>
#include <vector>

#include "../include/adt_hip.h"

// ---- the log ----------------------------------------------------------------------------------------------------------------------------------
struct Record { std::string text; std::vector<std::string> args; };      // one log line: its text without the argument bytes ; those
static bool g_verbose = false;
static std::vector<Record>* g_capture = nullptr;
static bool g_line_open = false;
static uint64_t g_shape, g_full;
static long g_launches;
static void log_reset() { g_shape = g_full = 1469598103934665603ull; g_launches = 0; }
static void hash_bytes(uint64_t& h, const void* p, size_t n) {
  const unsigned char* b = (const unsigned char*)p;
  for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
}
static void logf(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  int n = vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (n >= (int)sizeof buf) n = (int)sizeof buf - 1;
  hash_bytes(g_shape, buf, n);
  hash_bytes(g_full, buf, n);
  if (g_verbose) fputs(buf, stdout);
  if (g_capture) {
    if (!g_line_open) g_capture->push_back(Record{});
    g_capture->back().text.append(buf, n);
    g_line_open = n > 0 && buf[n - 1] != '\n';
  }
}
static void log_arg(int i, const void* p, size_t n) {
  logf(" arg%d[%zu]", i, n);
  hash_bytes(g_full, p, n);
  if (g_capture) g_capture->back().args.emplace_back((const char*)p, n);
  if (g_verbose) {
    fputc('=', stdout);
    for (size_t k = 0; k < n; ++k) printf("%02x", ((const unsigned char*)p)[k]);
  }
}

// ---- the HIP runtime, as much of it as the library imports --------------------------------------------------------------------------------------
struct dim3 { uint32_t x, y, z; };
typedef int hipError_t;
typedef void* hipStream_t;
typedef void* hipEvent_t;

static std::map<const void*, std::string> g_kernel_name;            // host stub -> device symbol (__hipRegisterFunction)
static std::map<std::string, std::vector<int>> g_arg_sizes;         // device symbol -> sizes of its explicit arguments
static int g_which = 0, g_streams[2], g_events[2];      // per loaded library: each creates its own side stream, and gets the same handles
static struct { dim3 grid, block; size_t smem; hipStream_t stream; } g_cfg_stack[8];
static int g_cfg_top = 0;
static int handle_index(const void* h) { return (int)((uintptr_t)h & 0xFFFF); }      // caller's stream: 1 ; created streams 0x101.. ; events 0x201..

extern "C" {
void** __hipRegisterFatBinary(const void*) { static void* module; return &module; }
void __hipUnregisterFatBinary(void**) {}
void __hipRegisterFunction(void**, const void* host_fn, char*, const char* device_name, unsigned, void*, void*, void*, void*, int*) { g_kernel_name[host_fn] = device_name; }
hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t smem, hipStream_t stream) {
  if (g_cfg_top >= 8) abort();
  g_cfg_stack[g_cfg_top++] = {grid, block, smem, stream};
  return 0;
}
hipError_t __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* smem, hipStream_t* stream) {
  if (g_cfg_top <= 0) abort();
  --g_cfg_top;
  *grid = g_cfg_stack[g_cfg_top].grid; *block = g_cfg_stack[g_cfg_top].block; *smem = g_cfg_stack[g_cfg_top].smem; *stream = g_cfg_stack[g_cfg_top].stream;
  return 0;
}
hipError_t hipLaunchKernel(const void* fn, dim3 grid, dim3 block, void** args, size_t smem, hipStream_t stream) {
  const auto name = g_kernel_name.find(fn);
  if (name == g_kernel_name.end()) { fprintf(stderr, "launch_log: launch of an unregistered kernel\n"); abort(); }
  const auto sizes = g_arg_sizes.find(name->second);
  if (sizes == g_arg_sizes.end()) { fprintf(stderr, "launch_log: no argument sizes for %s\n", name->second.c_str()); abort(); }
  ++g_launches;
  logf("launch %s grid %u %u %u block %u %u %u lds %zu stream %d", name->second.c_str(), grid.x, grid.y, grid.z, block.x, block.y, block.z, smem, handle_index(stream));
  for (size_t i = 0; i < sizes->second.size(); ++i) log_arg((int)i, args[i], (size_t)sizes->second[i]);
  logf("\n");
  return 0;
}
hipError_t hipFuncSetAttribute(const void* fn, int attr, int value) {
  logf("attribute %s %d %d\n", g_kernel_name.count(fn) ? g_kernel_name[fn].c_str() : "?", attr, value);
  return 0;
}
hipError_t hipGetLastError() { return 0; }
const char* hipGetErrorString(hipError_t) { return "launch_log: no error"; }
hipError_t hipGetDevice(int* dev) { *dev = 0; return 0; }
hipError_t hipDeviceGetAttribute(int* v, int, int) { *v = 256; return 0; }
hipError_t hipDeviceSynchronize() { return 0; }
hipError_t hipMalloc(void** p, size_t) { *p = nullptr; return 2; }      // (ADT_SEQ_STAMPS only: not part of the case list)
hipError_t hipMemcpy(void*, const void*, size_t, int) { return 1; }
hipError_t hipStreamIsCapturing(hipStream_t, int* status) { *status = 0; return 0; }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned flags) { *s = (void*)(uintptr_t)(0x50000100 + ++g_streams[g_which]); logf("stream create %d flags %u\n", handle_index(*s), flags); return 0; }
hipError_t hipStreamDestroy(hipStream_t s) { logf("stream destroy %d\n", handle_index(s)); return 0; }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned flags) { *e = (void*)(uintptr_t)(0x50000200 + ++g_events[g_which]); logf("event create %d flags %u\n", handle_index(*e), flags); return 0; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) { logf("event record %d stream %d\n", handle_index(e), handle_index(s)); return 0; }
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned) { logf("stream %d wait event %d\n", handle_index(s), handle_index(e)); return 0; }
}

// ---- the library --------------------------------------------------------------------------------------------------------------------------------
static void* g_lib;
#define ADT(name) ((decltype(&name))sym(#name))
static void* sym(const char* name) {
  void* p = dlsym(g_lib, name);
  if (!p) { fprintf(stderr, "launch_log: %s: %s\n", name, dlerror()); exit(2); }
  return p;
}
static int g_poison = 0;
__attribute__((noinline)) static void poison_stack() {
  volatile char buf[192 * 1024];
  memset((void*)buf, g_poison, sizeof buf);
  __asm__ volatile("" ::"r"(buf) : "memory");
}
static void ret(const char* what, long long rc) {
  logf("ret %s %lld%s%s\n", what, rc, rc < 0 ? " " : "", rc < 0 ? ADT(adt_last_error)() : "");
  poison_stack();
}
#define CALL(name, ...) (poison_stack(), ret(#name, ADT(name)(__VA_ARGS__)))

// made-up device addresses (16-byte aligned, far apart) and the arena of what the host layer reads
template <class T> static T* dev(int k) { return (T*)(uintptr_t)(0x700000000000ull + (uint64_t)k * 0x4000000000ull); }
struct Arena {
  adt_sasrec_cfg cfg;
  float lambdas1[16], lambdas2[16];
  adt_enc_layer_ptrs ep, eg;
  adt_dec_layer_ptrs dp, dg;
};
static Arena* g_arena;

static void run_config(int prec, int H, int L, int nl, int B) {
  Arena& A = *g_arena;
  A.cfg = adt_sasrec_cfg{3416, L, 64, H, nl, 0.5f, prec};
  const adt_sasrec_cfg* c = &A.cfg;
  float *P = dev<float>(1), *G = dev<float>(2), *ws = dev<float>(3), *M = dev<float>(4), *V = dev<float>(5), *scal = dev<float>(6), *norms = dev<float>(7);
  int32_t *seq = dev<int32_t>(8), *dec = seq + (size_t)B * L, *pos = dec + (size_t)B * L, *neg = pos + (size_t)B * L;
  uint32_t *seed = dev<uint32_t>(9), *state = dev<uint32_t>(10), *consumed = dev<uint32_t>(11), *produced = dev<uint32_t>(12);
  int32_t *ring = dev<int32_t>(13), *staging = dev<int32_t>(14), *cand = dev<int32_t>(15), *rank = dev<int32_t>(16);
  float* logits = dev<float>(17);
  void* st = (void*)(uintptr_t)0x50000001;
  const int64_t n_ints = 4 * (int64_t)B * L + 4, n = ADT(adt_sasrec_param_layout)(c, nullptr);
  const int nslots = 4;
  logf("config prec %d H %d L %d layers %d B %d\n", prec, H, L, nl, B);
  ret("adt_sasrec_workspace_floats", ADT(adt_sasrec_workspace_floats)(c, B));
  const int deferred = ADT(adt_sasrec_bce_deferred)(c);
  ret("adt_sasrec_bce_deferred", deferred);
  const int train = ADT_TRAIN_DROPOUT | ADT_TRAIN_PACKED;
  // the trainer's step (adt_amd/sasrec/trainer.py): form 0 single-GPU, 1 one exchange (ADT_DP_PHASES=1), 2 two buckets ; with and without the ring
  // prefetch ; the logits kernel left to the backward or launched by the forward
  for (int form = 0; form < 3; ++form)
    for (int prefetch = 0; prefetch < 2; ++prefetch)
      for (int side = 0; side < 2; ++side) {
        logf("step form %d prefetch %d side %d\n", form, prefetch, side);
        if (prefetch) CALL(adt_sasrec_step_begin_ring_staged, c, ws, B, seed, 0x9E3779B1u, ring, n_ints, nslots, seq, state, consumed, staging, produced, P, G, n, scal, st);
        else CALL(adt_sasrec_step_begin, c, ws, B, seed, 0x9E3779B1u, norms, P, G, n, scal, st);
        const bool pf = prefetch != 0;
        CALL(adt_sasrec_forward_loss_prefetch, c, P, ws, seq, dec, pos, neg, B, train | (side && deferred ? ADT_TRAIN_BCE_SIDE : 0), seed, 0u, A.lambdas1, A.lambdas2,
             pf ? ring : nullptr, pf ? n_ints : 0, pf ? nslots : 0, pf ? state : nullptr, pf ? consumed : nullptr, pf ? staging : nullptr, st);
        const int bce01 = !deferred ? 0 : (side ? ADT_PHASE_BCE_FWD : ADT_PHASE_BCE_HERE), bce2 = deferred ? ADT_PHASE_SEEDS_VIRTUAL : 0;
        const bool pb = pf && deferred && side;      // (only a forward that launched the logits kernel itself hands the ring on)
#define RING_ARGS pb ? ring : nullptr, pb ? n_ints : 0, pb ? nslots : 0, pb ? state : nullptr, pb ? consumed : nullptr, pb ? staging : nullptr
        if (form < 2) {
          CALL(adt_sasrec_backward_prefetch, c, P, G, ws, seq, dec, pos, neg, B, 1, seed, 0u, ADT_PHASE_PREZEROED | ADT_PHASE_DEFER_FOLD | bce01, RING_ARGS, st);
          if (form == 0) CALL(adt_sasrec_fold_clip_adam, c, ws, B, P, G, M, V, 0.01f, 1.0f, 1e-3f, 0.9f, 0.98f, 1e-8f, scal, st);
          else CALL(adt_sasrec_fold_grads, c, ws, B, P, G, scal, st);
        } else {
          CALL(adt_sasrec_backward_prefetch, c, P, G, ws, seq, dec, pos, neg, B, 1, seed, 0u, 1 | ADT_PHASE_PREZEROED | bce01, nullptr, 0, 0, nullptr, nullptr, nullptr, st);
          CALL(adt_sasrec_backward_prefetch, c, P, G, ws, seq, dec, pos, neg, B, 1, seed, 0u, 2 | ADT_PHASE_PREZEROED | bce2, RING_ARGS, st);
        }
      }
  // the other entry points: the unstaged ring, the plain training calls (a shard at an offset; no dropout), evaluation, the probe
  CALL(adt_sasrec_step_begin_ring, c, ws, B, seed, 0x9E3779B1u, ring, n_ints, nslots, seq, state, consumed, P, G, n, scal, st);
  CALL(adt_sasrec_forward, c, P, ws, seq, dec, pos, neg, B, ADT_TRAIN_DROPOUT, seed, 3u, st);
  CALL(adt_sasrec_loss_seed, c, ws, pos, B, A.lambdas1, A.lambdas2, st);
  CALL(adt_sasrec_backward, c, P, G, ws, seq, dec, pos, neg, B, 1, seed, 3u, 0, st);
  CALL(adt_sasrec_forward, c, P, ws, seq, dec, pos, neg, B, 0, seed, 0u, st);
  CALL(adt_sasrec_loss_seed_nz, c, ws, pos, B, A.lambdas1, A.lambdas2, st);
  CALL(adt_sasrec_backward, c, P, G, ws, seq, dec, pos, neg, B, 0, seed, 0u, 1, st);
  CALL(adt_sasrec_backward, c, P, G, ws, seq, dec, pos, neg, B, 0, seed, 0u, 2, st);
  CALL(adt_sasrec_forward_loss, c, P, ws, seq, dec, pos, neg, B, ADT_TRAIN_DROPOUT, seed, 0u, A.lambdas1, A.lambdas2, st);
  CALL(adt_sasrec_predict, c, P, ws, seq, cand, B, 101, logits, rank, st);
  CALL(adt_sasrec_probe_dec_layer_fwd, c, P, ws, dec, B, 1, seed, 0u, nl - 1, st);
  CALL(adt_sasrec_probe_dec_layer_fwd, c, P, ws, dec, B, 1, seed, 0u, nl, st);
  // rejected phase words, a rejected configuration
  for (int word : {3, ADT_PHASE_BCE_FWD, ADT_PHASE_BCE_FWD | ADT_PHASE_BCE_HERE | ADT_PHASE_PREZEROED, 2 | ADT_PHASE_BCE_FWD | ADT_PHASE_PREZEROED, ADT_PHASE_BCE_HERE})
    CALL(adt_sasrec_backward, c, P, G, ws, seq, dec, pos, neg, B, 1, seed, 0u, word, st);
  for (int bad = 0; bad < 4; ++bad) {
    adt_sasrec_cfg keep = A.cfg;
    if (bad == 0) A.cfg.hidden = 50;
    if (bad == 1) A.cfg.num_heads = 3;
    if (bad == 2) A.cfg.maxlen = 225;
    if (bad == 3) A.cfg.num_layers = 17;
    CALL(adt_sasrec_forward, c, P, ws, seq, dec, pos, neg, B, 0, seed, 0u, st);
    CALL(adt_sasrec_backward, c, P, G, ws, seq, dec, pos, neg, B, 0, seed, 0u, 0, st);
    CALL(adt_sasrec_fold_grads, c, ws, B, P, G, scal, st);
    ret("adt_sasrec_bce_deferred", ADT(adt_sasrec_bce_deferred)(c));
    A.cfg = keep;
  }
  // one layer per call
  const int hd = 64 / H;
  ret("adt_seq_layer_supported", ADT(adt_seq_layer_supported)(prec, L, 64, hd));
  ret("adt_seq_layer_supported", ADT(adt_seq_layer_supported)(prec, L, 128, hd));
  ret("adt_seq_layer_supported", ADT(adt_seq_layer_supported)(prec, L, 64, 0));
  float *x = dev<float>(18), *y = dev<float>(19), *save = dev<float>(20), *rec = dev<float>(21), *scratch = dev<float>(22), *feats = dev<float>(23), *gx = dev<float>(24);
  float *wp_base = dev<float>(25), *drec = dev<float>(26), *gfeats = dev<float>(27);
  void* wp_img = dev<void>(28);
  for (int training = 0; training < 2; ++training)
    CALL(adt_seq_enc_layer_fwd, B, L, H, seq, x, &A.ep, wp_base, wp_img, 0.5f, seed, 16u, 17u, 18u, 0u, training, save, y, 0.25f, training, rec, st);
  CALL(adt_seq_enc_layer_bwd, B, L, H, seq, x, &A.ep, &A.eg, wp_base, wp_img, 0.5f, seed, 16u, 17u, 18u, 0u, save, y, 0.25f, rec, drec, gx, 1, scratch, st);
  CALL(adt_seq_enc_layer_bwd, B, L, H, seq, x, &A.ep, &A.eg, wp_base, wp_img, 0.f, seed, 16u, 17u, 18u, 0u, save, y, 0.f, rec, nullptr, gx, 0, scratch, st);
  CALL(adt_seq_dec_layer_fwd, B, L, H, dec, x, feats, &A.dp, wp_base, wp_img, 0.5f, seed, 128u, 129u, 130u, 131u, 0u, save, y, 0.25f, 1, st);
  CALL(adt_seq_dec_layer_bwd, B, L, H, dec, x, feats, &A.dp, &A.dg, wp_base, wp_img, 0.5f, seed, 128u, 129u, 130u, 131u, 0u, save, y, 0.25f, gx, 1, gfeats, scratch, st);
}

// both libraries make the same calls: every record equal but for argument bytes, whose differing offsets are collected per kernel and argument
static std::map<std::pair<std::string, int>, std::map<int, long>> g_arg_diffs;
// The two argument structs with counted arrays (PackArgs, adt_wave.cuh: base, img, n, off[256] ; PartReduceArgs, adt_seq.hip: G, part, stride,
// nwg, nslots, slot[256], off[256], nwg_slot[256]): a difference in front of the arrays or inside their first `count` entries is a real one.
static const struct { const char* kernel; int count_at, arrays[3]; } COUNTED[] = {{"k_pack_wimg", 16, {20, -1, -1}}, {"k_dwpart_reduce", 28, {32, 1056, 2080}}};
static bool in_unused_tail(const std::string& kernel, const std::string& arg, size_t o) {
  for (const auto& c : COUNTED) {
    if (kernel.find(c.kernel) == std::string::npos) continue;
    int n;
    memcpy(&n, arg.data() + c.count_at, sizeof n);
    for (int base : c.arrays)
      if (base >= 0 && o >= (size_t)base + 4 * (size_t)n && o < (size_t)base + 4 * 256) return true;
    return o >= (size_t)(c.arrays[2] >= 0 ? c.arrays[2] : c.arrays[0]) + 4 * 256;      // padding behind the last array
  }
  return false;
}
// Padding of the argument structs the case list reaches, as [first, last] byte ranges of the FIRST argument (x86-64 layout: 4 bytes behind
// DropCfg::scale and behind an int in front of a pointer or size_t).  A differing byte anywhere else is an unequal record.
static const struct { const char* type; int ranges[5][2]; } PADDING[] = {
    {"BwdChainArgs", {{12, 15}, {44, 47}, {-1, -1}, {-1, -1}, {-1, -1}}},                    // T L B | ids ; drop (at 24)
    {"SeqFwdArgs", {{12, 15}, {44, 47}, {-1, -1}, {-1, -1}, {-1, -1}}},                      // L B H | ids ; drop (at 24)
    {"EmbedBwdArgs", {{28, 31}, {52, 55}, {60, 63}, {84, 87}, {100, 103}}},                  // scale | drop | row_offset | nrep | nslices
    {"EmbedBwd3Args", {{68, 71}, {92, 95}, {116, 119}, {124, 127}, {148, 151}}},             // scale | drop_s | drop_d | row_offset | nrep
    {"LogitsBceArgs", {{44, 47}, {108, 111}, {-1, -1}, {-1, -1}, {-1, -1}}},                 // T | nrep
    {"LogitsScatterArgs", {{12, 15}, {76, 79}, {92, 95}, {-1, -1}, {-1, -1}}},               // ldf | lddf | nrep
    {"RepReduce2Args", {{76, 79}, {-1, -1}, {-1, -1}, {-1, -1}, {-1, -1}}},                  // g0
};
static bool is_padding(const std::string& kernel, size_t k, size_t o) {
  if (k != 0) return false;
  const size_t params = kernel.find("Ev") != std::string::npos ? kernel.find("Ev") : 0;      // (the parameter list of a template kernel's symbol)
  size_t best = std::string::npos;
  const int (*ranges)[2] = nullptr;
  for (const auto& p : PADDING) {
    const size_t at = kernel.find(p.type, params);
    if (at != std::string::npos && at < best) { best = at; ranges = p.ranges; }
  }
  for (int i = 0; ranges && i < 5; ++i)
    if (ranges[i][0] >= 0 && o >= (size_t)ranges[i][0] && o <= (size_t)ranges[i][1]) return true;
  return false;
}
static long compare(const std::vector<Record>& a, const std::vector<Record>& b, const char* what) {
  long bad = 0;
  if (a.size() != b.size()) { printf("%s: %zu records against %zu\n", what, a.size(), b.size()); ++bad; }
  for (size_t i = 0; i < a.size() && i < b.size(); ++i) {
    if (a[i].text != b[i].text || a[i].args.size() != b[i].args.size()) {
      if (++bad <= 3) printf("%s: record %zu\n  %s  %s", what, i, a[i].text.c_str(), b[i].text.c_str());
      continue;
    }
    const std::string kernel = a[i].text.substr(0, a[i].text.find(" grid "));
    for (size_t k = 0; k < a[i].args.size(); ++k)
      for (size_t o = 0; o < a[i].args[k].size(); ++o)
        if (a[i].args[k][o] != b[i].args[k][o]) {
          ++g_arg_diffs[{kernel, (int)k}][(int)o];
          if (!in_unused_tail(kernel, a[i].args[k], o) && !is_padding(kernel, k, o) && ++bad <= 3)
            printf("%s: record %zu: argument %zu differs at byte %zu, which is neither padding nor an unused array tail\n  %s", what, i, k, o, a[i].text.c_str());
        }
  }
  return bad;
}

int main(int argc, char** argv) {
  if (argc != 4 && argc != 5 && argc != 9) { fprintf(stderr, "usage: %s <libadt_hip.so> <argsizes.txt> <poison byte> [<other libadt_hip.so> | prec H L layers B]\n", argv[0]); return 2; }
  FILE* f = fopen(argv[2], "r");
  if (!f) { perror(argv[2]); return 2; }
  char name[4096];
  int n;
  while (fscanf(f, "%4095s %d", name, &n) == 2) {
    std::vector<int> sizes(n);
    for (int i = 0; i < n; ++i)
      if (fscanf(f, "%d", &sizes[i]) != 1) return 2;
    g_arg_sizes[name] = sizes;
  }
  fclose(f);
  g_poison = atoi(argv[3]);
  g_arena = (Arena*)mmap((void*)0x600000000000ull, 1 << 20, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_FIXED_NOREPLACE, -1, 0);
  if (g_arena != (Arena*)0x600000000000ull) { perror("mmap"); return 2; }
  for (int i = 0; i < 16; ++i) { g_arena->lambdas1[i] = 0.5f + i; g_arena->lambdas2[i] = 0.25f + i; }
  float** ptrs = (float**)&g_arena->ep;      // the four layer pointer structs: 14 + 14 + 14 + 14 made-up device addresses
  for (int i = 0; i < 56; ++i) ptrs[i] = dev<float>(40 + i);
  log_reset();
  g_lib = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (!g_lib) { fprintf(stderr, "launch_log: %s\n", dlerror()); return 2; }
  if (argc == 9) {
    g_verbose = true;
    run_config(atoi(argv[4]), atoi(argv[5]), atoi(argv[6]), atoi(argv[7]), atoi(argv[8]));
    return 0;
  }
  void* const first = g_lib;
  void* const other = argc == 5 ? dlopen(argv[4], RTLD_NOW | RTLD_LOCAL) : nullptr;
  if (argc == 5 && !other) { fprintf(stderr, "launch_log: %s\n", dlerror()); return 2; }
  long configs = 0, launches = 0, bad = 0;
  for (int prec = 0; prec < 2; ++prec)
    for (int H : {1, 2, 4})
      for (int L : {8, 50, 200, 202, 224})
        for (int nl : {1, 2, 3, 5})
          for (int B : {1, 8, 32, 128, 256}) {
            std::vector<Record> a, b;
            log_reset();
            g_capture = other ? &a : nullptr;
            run_config(prec, H, L, nl, B);
            ++configs; launches += g_launches;
            if (!other) { printf("%d %d %d %d %d %ld %016llx %016llx\n", prec, H, L, nl, B, g_launches, (unsigned long long)g_shape, (unsigned long long)g_full); continue; }
            g_lib = other; g_which = 1; g_capture = &b;
            run_config(prec, H, L, nl, B);
            g_lib = first; g_which = 0; g_capture = nullptr;
            char what[64];
            snprintf(what, sizeof what, "%d %d %d %d %d", prec, H, L, nl, B);
            bad += compare(a, b, what);
          }
  if (other) {
    printf("configs %ld launches %ld unequal-records %ld\n", configs, launches, bad);
    for (const auto& d : g_arg_diffs) {
      printf("argdiff %s arg%d", d.first.first.c_str(), d.first.second);
      for (const auto& o : d.second) printf(" %d", o.first);
      printf("\n");
    }
  }
  return 0;
}
