// Host half of every kernel launch of the project -- the denoiser (libprd_hip.so) and the five side libraries (prd_align.hip,
// prd_tmalign.hip, prd_quality.hip, prd_condition.hip, prd_sequence.hip): the checked launch, the raise of a kernel's dynamic-LDS limit,
// the memset ahead of a launch, the pair_dim dispatch and the launch geometry.  Host code only -- nothing here reaches a kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <mutex>

// ---- 1. the launch ---------------------------------------------------------------------------------------------------------------
// Dynamic LDS up to PRD_LDS_DEFAULT_LIMIT needs no attribute; a launch that asks for more first raises the kernel's limit to the
// hardware maximum less the kernel's static LDS, once per process and kernel (thread-safe: std::call_once; not a stream operation, so
// it is legal during hipGraph capture).  The result of the raise is kept: if it failed, nothing is launched and every call returns that
// error.  prd_launch makes the raise itself; an entry point with several launches calls prd_lds_ready ahead of its first one, so that
// a refusal leaves nothing launched.  PRD_LDS_MAX is the one limit raised to: a source whose kernels take dynamic LDS shows that its
// largest size fits, with room for whatever the kernel declares statically.
constexpr size_t PRD_LDS_DEFAULT_LIMIT = 48 * 1024;
constexpr int PRD_LDS_MAX = 160 * 1024;

// an entry point with several launches returns the first non-zero result and launches nothing after it
#define PRD_TRY(launch)                                                                                         \
    do {                                                                                                        \
        const int prd_e_ = (launch);                                                                            \
        if (prd_e_) return prd_e_;                                                                              \
    } while (0)

#ifdef PRD_LAUNCH_TRACE
// The trace build (build.py: variant "trace"; tests/native/launch_trace.c for the denoiser, side_launch_trace.c for the side libraries): a
// launch prints one line -- kernel, grid, block, LDS bytes and every argument (integers and floats by value, pointers by address,
// structures as their bytes in hex) -- and returns 0; the raise is a no-op and the memset a line of its own.  No HIP function is
// called, so every host decision above a launch can be compared between two trees on a machine without a GPU.
#include <cxxabi.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <typeinfo>
template <class T>
static void prd_trace_arg(const T& v) {
    if constexpr (std::is_pointer_v<T> || std::is_null_pointer_v<T>) printf(" %p", (const void*)v);
    else if constexpr (std::is_floating_point_v<T>) printf(" %.9g", (double)v);
    else if constexpr (std::is_integral_v<T> || std::is_enum_v<T>) printf(" %lld", (long long)v);
    else {
        unsigned char bytes[sizeof(T)];
        memcpy(bytes, &v, sizeof(T));
        printf(" {");
        for (size_t i = 0; i < sizeof(T); ++i) printf("%02x", bytes[i]);
        printf("}");
    }
}
template <auto Kernel, class... Args>
static int prd_launch(dim3 grid, dim3 block, size_t lds, hipStream_t, Args... args) {
    // the kernel with its template arguments: the mangled name of a type local to this instantiation holds the kernel's own
    // ("...XadL_Z<kernel>EE...E4Here"), whose shortest piece that demangles is "[(anonymous namespace)::]name<arguments>"; a kernel
    // that is no template and lies in no namespace is "_Z<length><name><parameters>"
    struct Here {};
    const char* mangled = strstr(typeid(Here).name(), "XadL_Z");
    char piece[1024] = "?";
    char* full = nullptr;
    int plain = 0, at = 0;
    if (mangled && sscanf(mangled + 6, "%d%n", &plain, &at) == 1 && mangled[6 + at + plain] != 'I') {
        snprintf(piece, sizeof piece, "%.*s", plain, mangled + 6 + at);
    } else if (mangled) {
        const char* start = mangled + 4;
        for (const char* e = strchr(start, 'E'); e && !full; e = strchr(e + 1, 'E')) {
            snprintf(piece, sizeof piece, "%.*s", (int)(e + 1 - start), start);
            full = abi::__cxa_demangle(piece, nullptr, nullptr, nullptr);
        }
    }
    const char* name = full ? full : piece;
    if (!strncmp(name, "(anonymous namespace)::", 23)) name += 23;
    const int len = (int)strlen(name);
    printf("L %.*s grid %u %u %u block %u %u %u lds %zu args", len, name, grid.x, grid.y, grid.z, block.x, block.y, block.z, lds);
    (prd_trace_arg(args), ...);
    printf("\n");
    free(full);
    return 0;
}
template <auto Kernel>
static int prd_lds_ready(size_t) {
    return 0;
}
// the memset that precedes a launch: one line "M address value bytes"
static int prd_memset_async(void* ptr, int value, size_t bytes, hipStream_t) {
    printf("M %p %d %zu\n", ptr, value, bytes);
    return 0;
}
#else
// Kernel may be launched with lds bytes of dynamic LDS: 0, or the kept hipError_t of the raise
template <auto Kernel>
static int prd_lds_ready(size_t lds) {
    if (lds <= PRD_LDS_DEFAULT_LIMIT) return 0;
    static std::once_flag once;
    static hipError_t raised = hipSuccess;
    std::call_once(once, [] {           // static and dynamic LDS share the 160 KiB: a limit that leaves the static part no room is refused
        hipFuncAttributes attr;
        raised = hipFuncGetAttributes(&attr, (const void*)Kernel);
        if (raised == hipSuccess)
            raised = hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, PRD_LDS_MAX - (int)attr.sharedSizeBytes);
    });
    return (int)raised;
}
// launches Kernel<<<grid, block, lds, stream>>>(args...); returns 0 or the hipError_t of the raise / the launch
template <auto Kernel, class... Args>
static int prd_launch(dim3 grid, dim3 block, size_t lds, hipStream_t stream, Args... args) {
    PRD_TRY(prd_lds_ready<Kernel>(lds));
    hipLaunchKernelGGL(Kernel, grid, block, lds, stream, args...);
    return (int)hipGetLastError();
}
// the memset that precedes a launch
static int prd_memset_async(void* ptr, int value, size_t bytes, hipStream_t stream) {
    return (int)hipMemsetAsync(ptr, value, bytes, stream);
}
#endif

// ---- 2. run-time value -> compile-time constant ------------------------------------------------------------------------------------
// PRD_FOR_P(P, PP, expr) evaluates expr once with `constexpr int PP` bound to 64 or 32 (pair_dim is validated by the caller), so a
// launch is written once:  return PRD_FOR_P(P, PP, prd_launch<kernel<PP, 8>>(grid, block, lds, stream, ...));
// A second choice nests:   PRD_FOR_P(P, PP, PRD_FOR_BOOL(b3, B3, prd_launch<kernel<PP, B3>>(...)))
#define PRD_WITH(T, NAME, VALUE, ...) [&] { constexpr T NAME = VALUE; return __VA_ARGS__; }()
// v is A or anything else (-> B)
#define PRD_FOR_2(v, NAME, A, B, ...) ((v) == (A) ? PRD_WITH(int, NAME, A, __VA_ARGS__) : PRD_WITH(int, NAME, B, __VA_ARGS__))
#define PRD_FOR_P(P, PP, ...) PRD_FOR_2(P, PP, 64, 32, __VA_ARGS__)
#define PRD_FOR_BOOL(v, NAME, ...) ((v) ? PRD_WITH(bool, NAME, true, __VA_ARGS__) : PRD_WITH(bool, NAME, false, __VA_ARGS__))
// v is A, B or anything else (-> C)
#define PRD_FOR_3(v, NAME, A, B, C, ...) \
    ((v) == (A) ? PRD_WITH(int, NAME, A, __VA_ARGS__) : (v) == (B) ? PRD_WITH(int, NAME, B, __VA_ARGS__) : PRD_WITH(int, NAME, C, __VA_ARGS__))

// ---- 3. launch geometry ------------------------------------------------------------------------------------------------------------
// persistent workgroups over a task queue: per_wg tasks per workgroup, between 1 and cap workgroups
static inline int grid_for(long tasks, int per_wg, int cap) {
    long g = (tasks + per_wg - 1) / per_wg;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (int)g;
}

// persistent workgroups over the rows of one head (grid = result * H; cap = workgroups a head may have): the SMALLEST count that
// reaches the minimum number of row rounds, so every workgroup walks the same number of rows
static inline long prd_rows_per_head(long rows_total, long cap) {
    long per_head = cap < rows_total ? cap : rows_total;
    if (per_head < 1) per_head = 1;
    const long rounds = (rows_total + per_head - 1) / per_head;
    return (rows_total + rounds - 1) / rounds;
}

// the same, as a multiple of 8 rows in flight per head (never more rounds, never above cap): the kernels then keep the head-workgroups
// of a row on ONE XCD, whose L2 serves the row to all of them.  (N = 769, H = 4: 60 -> 64 rows in flight.)  xcd8 = false: the A/B
// switch PRD_TUNE_TA2_NO_XCD8
static inline long prd_rows_per_head_xcd8(long rows_total, long cap, bool xcd8 = true) {
    long per_head = prd_rows_per_head(rows_total, cap);
    if (per_head >= 8 && xcd8) per_head = (per_head + 7) / 8 * 8;
    if (per_head > cap) per_head = cap;
    return per_head;
}
