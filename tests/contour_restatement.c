/* The plain-C twin of dsdtm_amd/contour_restatement.py: rules C1-C5 of include/dsdtm_amd_mcd.h, sequentially — a raster scan, a flood
 * fill and a Moore trace per component, no pruning, no union-find. Test infrastructure (tests/test_mcd_cpu.py); integer only. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

static const int DX[8] = {1, 1, 0, -1, -1, -1, 0, 1};
static const int DY[8] = {0, -1, -1, -1, 0, 1, 1, 1};

static int on(const uint8_t* m, int w, int h, int stride, int x, int y) {
    return x >= 0 && x < w && y >= 0 && y < h && m[(size_t)y * (size_t)stride + (size_t)x] != 0;
}

/* C2 + C3 for the component whose raster-first pixel is (x0, y0): area2 and the border's extents; -1 when the walk passes its cap */
static int trace(const uint8_t* m, int w, int h, int stride, int x0, int y0, int64_t* area2, int ext[4]) {
    int s = 4, x = x0, y = y0, x1, y1;
    int64_t acc = 0, left = 4 * (int64_t)w * h + 4;
    ext[0] = ext[2] = x0; ext[1] = ext[3] = y0;
    *area2 = 0;
    do { s = (s - 1) & 7; } while (!on(m, w, h, stride, x0 + DX[s], y0 + DY[s]) && s != 4);
    if (s == 4) return 0;
    x1 = x0 + DX[s]; y1 = y0 + DY[s];
    for (;;) {
        int nx, ny;
        if (--left < 0) return -1;
        do { s = (s + 1) & 7; nx = x + DX[s]; ny = y + DY[s]; } while (!on(m, w, h, stride, nx, ny));
        acc += (int64_t)x * ny - (int64_t)y * nx;
        if (x < ext[0]) ext[0] = x;
        if (y < ext[1]) ext[1] = y;
        if (x > ext[2]) ext[2] = x;
        if (y > ext[3]) ext[3] = y;
        if (nx == x0 && ny == y0 && x == x1 && y == y1) break;
        x = nx; y = ny; s = (s + 4) & 7;
    }
    *area2 = acc < 0 ? -acc : acc;
    return 0;
}

/* box: x, y, w, h (all 0: nothing drawn); boxed may be NULL. Returns 0, or -1 (no memory, a walk past its cap). */
int contour_box(const uint8_t* mask, int w, int h, int stride, uint8_t* boxed, int boxed_stride, int32_t box[4], int64_t* area2, int32_t* n_components) {
    const size_t pixels = (size_t)w * (size_t)h;
    uint8_t* seen = (uint8_t*)calloc(pixels, 1);
    int32_t* stack = (int32_t*)malloc(pixels * sizeof(int32_t));
    int64_t best = 0;
    int best_ext[4] = {0, 0, -1, -1}, count = 0, rc = 0;
    if (!seen || !stack) { free(seen); free(stack); return -1; }
    for (int y0 = 0; y0 < h && rc == 0; ++y0)
        for (int x0 = 0; x0 < w; ++x0) {
            size_t top = 0;
            int64_t a2;
            int ext[4];
            if (!on(mask, w, h, stride, x0, y0) || seen[(size_t)y0 * w + x0]) continue;
            ++count;
            seen[(size_t)y0 * w + x0] = 1;
            stack[top++] = y0 * w + x0;
            while (top) {
                const int p = stack[--top], cx = p % w, cy = p / w;
                for (int k = 0; k < 8; ++k) {
                    const int nx = cx + DX[k], ny = cy + DY[k];
                    if (on(mask, w, h, stride, nx, ny) && !seen[(size_t)ny * w + nx]) { seen[(size_t)ny * w + nx] = 1; stack[top++] = ny * w + nx; }
                }
            }
            if (trace(mask, w, h, stride, x0, y0, &a2, ext) != 0) { rc = -1; break; }
            if (a2 > best) { best = a2; memcpy(best_ext, ext, sizeof ext); }       /* C4 */
        }
    free(seen); free(stack);
    if (rc != 0) return rc;
    box[0] = box[1] = box[2] = box[3] = 0;
    if (best > 0) { box[0] = best_ext[0]; box[1] = best_ext[1]; box[2] = best_ext[2] - best_ext[0] + 1; box[3] = best_ext[3] - best_ext[1] + 1; }
    *area2 = best;
    *n_components = count;
    if (boxed)
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                const int in = best > 0 && x >= best_ext[0] && x <= best_ext[2] && y >= best_ext[1] && y <= best_ext[3];       /* C5 */
                boxed[(size_t)y * (size_t)boxed_stride + (size_t)x] = in ? 255 : mask[(size_t)y * (size_t)stride + (size_t)x];
            }
    return 0;
}
