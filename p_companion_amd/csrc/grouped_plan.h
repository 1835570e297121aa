// What the type-grouped catalogue kernels share (retrieve.hip: the top n of a type; rank.hip: the rank of one product in it):
// the chunk and slice constants, the slice plan and the total order of (score, product).
#pragma once

#define RG_NONE 0x7fffffff
#define RG_AUTO_SLICES 16
#define RG_MAX_SLICES 64
#define RG_SLICE_MIN 4096          // candidates a slice gets at least (fewer slices for a small type)
#define RG_CHUNK 64                // candidates per chunk: four waves x 16
#define RG_MAX_GRID 4096

// Slices of a type with C candidates at most S slices: ns slices of L candidates (L a multiple of the chunk, the last slice
// shorter), none empty.  Host and device use the same arithmetic.
__host__ __device__ __forceinline__ void rg_slice_plan(int C, int S, int& ns, int& L) {
    if (C <= 0) { ns = 0; L = 0; return; }
    int want = (C + RG_SLICE_MIN - 1) / RG_SLICE_MIN;
    if (want > S) want = S;
    const int per = (C + want - 1) / want;
    L = (per + RG_CHUNK - 1) / RG_CHUNK * RG_CHUNK;
    ns = (C + L - 1) / L;
}

// (score descending, product index ascending)
__device__ __forceinline__ bool rg_better(float x, int xi, float y, int yi) { return x > y || (x == y && xi < yi); }
