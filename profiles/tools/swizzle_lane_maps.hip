#include <hip/hip_runtime.h>
#include <cstdio>
__global__ void k(int *out)
{
    const int x = threadIdx.x;
    out[x] = __builtin_amdgcn_ds_swizzle(x, 0xC000 | (0 << 10) | (4 << 5));
    out[64 + x] = __builtin_amdgcn_ds_swizzle(x, 0xC000 | (1 << 10) | (4 << 5));
    out[128 + x] = __builtin_amdgcn_ds_swizzle(x, 0x8000 | 1 | (2 << 2) | (3 << 4) | (3 << 6));
    out[192 + x] = __builtin_amdgcn_ds_swizzle(x, 0x8000 | 0 | (0 << 2) | (1 << 4) | (2 << 6));
}
int main()
{
    int *d, h[256];
    if (hipMalloc(&d, sizeof(h)) != hipSuccess) return 1;
    hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, 0, d);
    if (hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return 2;
    for (int r = 0; r < 4; ++r) { for (int i = 0; i < 64; ++i) printf("%d ", h[64 * r + i]); printf("\n"); }
    return 0;
}
