/*
 * tests/golden/view_ref_main.c -- TEST INFRASTRUCTURE ONLY. A driver, linked by make_view_fixtures.py
 * against the REFERENCE's own radiosityNative.o / rectangle.o / vector3_cl.o (oracle/_ref/obj, compiled
 * by oracle/build_ref.sh), that casts one ray per pixel of a pin-hole camera through the reference's
 * getSortedIntersectableRects and findClosestIntersectionSorted (radiosityNative.c:25-90) over the walls
 * of a FMGIGEO1 geometry fixture. Every arithmetic step is a call of a reference function; this file only
 * loops, counts and writes.
 *
 *   view_ref <geometry.bin> <out.bin> <W> <H> <10 hex words: pos xyz, dir xyz, up xyz, pixel as float bits>
 *
 * out.bin: int32 {candidates, W, H}; per candidate int32 wall index (found through lightmapSetup.s0) and
 * the float bits of its minDistance; per pixel int32 wall, then per pixel int32 texel, then per pixel the
 * float bits of the hit distance; int64 number of intersects() evaluations (a second walk of the list).
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rectangle.h"
#include "vector3_cl.h"

/* radiosityNative.c keeps this type and the two functions to itself; the layout is {Rectangle, float} */
typedef struct RectInfo {
    Rectangle rect;
    float minDistance;
} RectInfo;
int getSortedIntersectableRects(Rectangle *rectsIn, int numRectsIn, Vector3 camPos, Vector3 camDir, RectInfo **rectsOut);
Rectangle *findClosestIntersectionSorted(Vector3 rayPos, Vector3 rayDir, RectInfo *rects, int numRects, float *dist);

static float from_bits(const char *hex) {
    uint32_t u = (uint32_t)strtoul(hex, NULL, 16);
    float f;
    memcpy(&f, &u, 4);
    return f;
}

static int32_t bits_of(float f) {
    int32_t u;
    memcpy(&u, &f, 4);
    return u;
}

static int wall_of(const Rectangle *walls, int n, const Rectangle *r) {
    for (int i = 0; i < n; i++)
        if (walls[i].lightmapSetup.s[0] == r->lightmapSetup.s[0]) return i;
    return -1;
}

int main(int argc, char **argv) {
    if (argc != 15) {
        fprintf(stderr, "usage: %s geometry.bin out.bin W H <10 float-bit hex words>\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    char magic[8];
    int hdr[4]; /* windows, lights, walls, texels */
    if (fread(magic, 1, 8, f) != 8 || memcmp(magic, "FMGIGEO1", 8) || fread(hdr, sizeof hdr, 1, f) != 1) return 4;
    const size_t n = (size_t)hdr[0] + hdr[1] + hdr[2];
    Rectangle *all = NULL;
    if (posix_memalign((void **)&all, 16, (n ? n : 1) * sizeof(Rectangle))) return 5;
    if (fread(all, sizeof(Rectangle), n, f) != n) return 6;
    fclose(f);
    Rectangle *walls = all + hdr[0] + hdr[1];
    const int numWalls = hdr[2];
    const int W = atoi(argv[3]), H = atoi(argv[4]);
    float v[10];
    for (int i = 0; i < 10; i++) v[i] = from_bits(argv[5 + i]);
    const Vector3 camPos = createVector3(v[0], v[1], v[2]);
    const Vector3 camUp = createVector3(v[6], v[7], v[8]);
    const float pixel = v[9];

    const Vector3 camDir = normalized(createVector3(v[3], v[4], v[5]));
    const Vector3 screenCenter = add(camPos, camDir);
    const Vector3 camRight = cross(camDir, camUp);
    RectInfo *rects = NULL;
    const int numRects = getSortedIntersectableRects(walls, numWalls, camPos, camDir, &rects);

    const size_t pix = (size_t)W * H;
    int32_t *wall = malloc(pix * 4 + 4), *texel = malloc(pix * 4 + 4), *dbits = malloc(pix * 4 + 4);
    int32_t *cand = malloc((size_t)numRects * 8 + 8);
    if (!wall || !texel || !dbits || !cand) return 7;
    for (int i = 0; i < numRects; i++) {
        cand[2 * i] = wall_of(walls, numWalls, &rects[i].rect);
        cand[2 * i + 1] = bits_of(rects[i].minDistance);
    }
    int64_t tests = 0;
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const Vector3 screenPos =
                add3(screenCenter, mul(camRight, pixel * (x - W / 2)), mul(camUp, -pixel * (y - H / 2)));
            const Vector3 rayDir = normalized(sub(screenPos, camPos));
            float dist = INFINITY;
            Rectangle *hit = findClosestIntersectionSorted(camPos, rayDir, rects, numRects, &dist);
            const size_t o = (size_t)y * W + x;
            wall[o] = hit ? wall_of(walls, numWalls, hit) : -1;
            texel[o] = hit ? hit->lightmapSetup.s[0] + getTileIdAt(hit, add(camPos, mul(rayDir, dist))) : -1;
            dbits[o] = bits_of(dist);
            /* the same walk again, counting the reference's intersects() calls */
            float d = INFINITY;
            for (int i = 0; i < numRects; i++) {
                if (d < rects[i].minDistance) break;
                tests++;
                const float dn = intersects(&rects[i].rect, camPos, rayDir, d);
                if (dn < 0) continue;
                if (dn <= d) d = dn;
            }
            if (bits_of(d) != bits_of(dist)) return 8;
        }
    FILE *o = fopen(argv[2], "wb");
    if (!o) return 9;
    const int32_t head[3] = {numRects, W, H};
    if (fwrite(head, 4, 3, o) != 3 || fwrite(cand, 8, (size_t)numRects, o) != (size_t)numRects ||
        fwrite(wall, 4, pix, o) != pix || fwrite(texel, 4, pix, o) != pix || fwrite(dbits, 4, pix, o) != pix ||
        fwrite(&tests, 8, 1, o) != 1)
        return 10;
    fclose(o);
    return 0;
}
