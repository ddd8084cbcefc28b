// components.hip — connected components of the unitig graph, on the GPU (gfx950).  Input: the device arrays of a unitig list (unitigs.hip): the unitig edges'
// n1 / n2 and the per-unitig offsets, length, kc_sum, circular.  Definition: include/mdbg_hip.h (mdbg_graph_components).
//
//   init_kernel      parent[u] = u, the per-component sums zeroed
//   hook_kernel      one thread per unitig edge record: a lock-free union-find.  Find the two roots, link the LARGER root under the smaller by a compare-and-swap
//                    on parent[larger]; a lost race continues from the value the CAS returned.  Finds halve the path as they go.
//                    Invariant: parent[x] <= x always, and parent[x] is only ever replaced by an ancestor of x.  So chains strictly descend (a find ends within
//                    n_unitigs steps), a vertex that stopped being a root never becomes one again, every record's CAS fails at most once per link made
//                    (n_unitigs - 1 in all), and the last root of a component is its smallest unitig number.
//   flatten_kernel   root[u] = find(u), is_root[u]
//   (rocPRIM)        exclusive scan of is_root: the rank of a root = the number of its component (components are numbered by their smallest unitig)
//   sum_kernel       component[u] = rank[root[u]]; integer atomics add the unitig's entries, bases and abundance to its component, the root writes first_unitig
//
// Every access to parent[] in the hook and flatten kernels is an agent-scope relaxed atomic: the eight XCDs of the device have L2s of their own, and a plain load
// may go on returning parent[x] == x from its own cache after a workgroup on another XCD linked x — a CAS against a re-read that never changes would fail for ever.
// All sums are integers and the roots are minima: the result does not depend on the order in which the records are hooked.
// No loop is unbounded (cap: n_unitigs + 1 steps; running into it sets status[0], reported as a defect by the host, never waited on), and the number of launches is fixed.
#include <cstring>

#include "components.h"
#include "graph_common.h"

struct ComponentBuffers {
    Buf parent, root, isroot, rank, tmp, status;
    Buf component, first, unitigs, nodes, bases, kc, circ;      // the result
};

namespace {

#define RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

struct CompArgs {
    u64 U, E; const u32* n1; const u32* n2; const u64* offsets; const u64* length; const u64* kc_in; const u8* circ_in;
    u32* parent; u32* root; u32* isroot; const u32* rank; u32* status;
    u32* component; u32* first; u32* unitigs; u64* nodes; u64* bases; u64* kc; u32* circ_words;
};

__device__ inline void set_defect(u32* status) { __hip_atomic_store(status, 1u, RLX_AGENT); }

// the root of x's tree as it stands; halves the path on the way (parent[x] <- its grandparent: an ancestor, smaller than parent[x]).  0xFFFFFFFF: the bound was hit (status[0] set)
__device__ inline u32 find_root(u32* parent, u32 x, u32 cap, u32* status) {
    u32 p = __hip_atomic_load(parent + x, RLX_AGENT);
    for (u32 i = 0; p != x; ++i) {
        if (i >= cap) { set_defect(status); return 0xFFFFFFFFu; }
        const u32 g = __hip_atomic_load(parent + p, RLX_AGENT);
        if (g != p) __hip_atomic_store(parent + x, g, RLX_AGENT);
        x = p; p = g;
    }
    return x;
}

__global__ __launch_bounds__(256) void init_kernel(CompArgs a) {
    const u64 u = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= a.U) return;
    a.parent[u] = (u32)u;
    a.unitigs[u] = 0; a.nodes[u] = 0; a.bases[u] = 0; a.kc[u] = 0;
    if ((u & 3) == 0) a.circ_words[u >> 2] = 0;
}

__global__ __launch_bounds__(256) void hook_kernel(CompArgs a) {
    const u64 e = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.E) return;
    u32 x = a.n1[e], y = a.n2[e];
    if (x >= a.U || y >= a.U) { set_defect(a.status); return; }      // a record of another list: never index outside
    if (x == y) return;                                              // "u + u +": joins nothing
    const u32 cap = (u32)a.U + 1;
    for (u32 tries = 0;; ++tries) {
        if (tries >= cap) { set_defect(a.status); return; }
        x = find_root(a.parent, x, cap, a.status);
        y = find_root(a.parent, y, cap, a.status);
        if (x == y || x >= a.U || y >= a.U) return;
        const u32 hi = x > y ? x : y, lo = x > y ? y : x;
        u32 seen = hi;
        if (__hip_atomic_compare_exchange_strong(a.parent + hi, &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
        x = seen; y = lo;                                            // somebody else linked hi meanwhile: go on from where it points now
    }
}

__global__ __launch_bounds__(256) void flatten_kernel(CompArgs a) {
    const u64 u = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= a.U) return;
    const u32 r = find_root(a.parent, (u32)u, (u32)a.U + 1, a.status);
    a.root[u] = r; a.isroot[u] = r == (u32)u ? 1u : 0u;                 // (a find that hit its bound leaves 0xFFFFFFFF: sum_kernel skips it, the host reports the defect)
}

__global__ __launch_bounds__(256) void sum_kernel(CompArgs a) {
    const u64 u = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= a.U) return;
    const u32 r = a.root[u];
    if (u == a.U - 1) a.status[1] = a.rank[u] + a.isroot[u];         // the scan's total: the number of components
    if (r >= a.U) { set_defect(a.status); return; }
    const u32 c = a.rank[r];
    if (c >= a.U) { set_defect(a.status); return; }
    a.component[u] = c;
    if (r == (u32)u) a.first[c] = (u32)u;
    atomicAdd(a.unitigs + c, 1u);
    atomicAdd((unsigned long long*)(a.nodes + c), (unsigned long long)(a.offsets[u + 1] - a.offsets[u]));
    atomicAdd((unsigned long long*)(a.bases + c), (unsigned long long)a.length[u]);
    atomicAdd((unsigned long long*)(a.kc + c), (unsigned long long)a.kc_in[u]);
    if (a.circ_in[u]) atomicOr(a.circ_words + (c >> 2), 1u << (8 * (c & 3)));      // byte c of the u8 array
}

}  // namespace

ComponentBuffers* component_buffers_create() { return new ComponentBuffers(); }
void component_buffers_destroy(ComponentBuffers* b) { delete b; }

hipError_t queue_components(ComponentBuffers* B, const UnitigResult& ul, hipStream_t s, ComponentResult* out) {
    memset(out, 0, sizeof *out);
    const u64 U = ul.n_unitigs, E = ul.edges.n;
    if (U == 0) return hipSuccess;
    if (U >= (1ull << 31) || E >= (1ull << 32)) return hipErrorInvalidValue;      // (unitigs.hip never makes such a list: u32 labels)
    GHIP(B->status.ensure(16));
    GHIP(hipMemsetAsync(B->status.p, 0, 16, s));
    GHIP(B->parent.ensure(U * 4)); GHIP(B->root.ensure(U * 4)); GHIP(B->isroot.ensure(U * 4)); GHIP(B->rank.ensure(U * 4));
    GHIP(B->component.ensure(U * 4)); GHIP(B->first.ensure(U * 4)); GHIP(B->unitigs.ensure(U * 4)); GHIP(B->nodes.ensure(U * 8)); GHIP(B->bases.ensure(U * 8));
    GHIP(B->kc.ensure(U * 8)); GHIP(B->circ.ensure((U + 3) / 4 * 4));
    CompArgs a; memset(&a, 0, sizeof a);
    a.U = U; a.E = E; a.n1 = ul.edges.n1; a.n2 = ul.edges.n2; a.offsets = ul.offsets; a.length = ul.length; a.kc_in = ul.kc_sum; a.circ_in = ul.circular;
    a.parent = B->parent.as<u32>(); a.root = B->root.as<u32>(); a.isroot = B->isroot.as<u32>(); a.rank = B->rank.as<u32>(); a.status = B->status.as<u32>();
    a.component = B->component.as<u32>(); a.first = B->first.as<u32>(); a.unitigs = B->unitigs.as<u32>(); a.nodes = B->nodes.as<u64>(); a.bases = B->bases.as<u64>();
    a.kc = B->kc.as<u64>(); a.circ_words = B->circ.as<u32>();
    const unsigned gu = grid_for(U);
    hipLaunchKernelGGL(init_kernel, dim3(gu), dim3(256), 0, s, a);
    if (E) hipLaunchKernelGGL(hook_kernel, dim3(grid_for(E)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(flatten_kernel, dim3(gu), dim3(256), 0, s, a);
    GHIP(excl_scan(B->tmp, B->isroot.as<u32>(), B->rank.as<u32>(), (size_t)U, s));
    hipLaunchKernelGGL(sum_kernel, dim3(gu), dim3(256), 0, s, a);
    out->n_unitigs = U; out->component = a.component; out->first_unitig = a.first; out->unitigs = a.unitigs; out->nodes = a.nodes; out->bases = a.bases; out->kc_sum = a.kc;
    out->circular = B->circ.as<u8>(); out->status = a.status;
    return hipGetLastError();
}

hipError_t build_components(ComponentBuffers* B, const UnitigResult& ul, hipStream_t s, ComponentResult* out, int* broken) {
    *broken = 0;
    GHIP(queue_components(B, ul, s, out));
    if (out->n_unitigs == 0) return hipSuccess;
    u32 st[2] = {0, 0};
    GHIP(hipMemcpyAsync(st, out->status, 8, hipMemcpyDeviceToHost, s));
    GHIP(hipStreamSynchronize(s));
    if (st[0] || st[1] == 0 || st[1] > out->n_unitigs) { memset(out, 0, sizeof *out); *broken = 1; return hipSuccess; }
    out->n_components = st[1];
    return hipSuccess;
}
