/* huffman_decoder -- CLI-compatible replacement for the reference's src/huffman_decoder.c
 * (huffman_decoder.c:39-99,170-305): decodes <template>huffman_indices.bin on the GPU.
 *   huffman_decoder <huffman output template> [--output-file f] [--check-file pq] [--tree]
 *                   [--rows FIRST:COUNT]
 * --output-file writes the raw n x m codes (no header), as the reference does.
 * --check-file is a real check: both sides are put in the encoder's sort order and
 * compared byte by byte (the reference's strncmp compare is vacuous).
 * --rows FIRST:COUNT (pqh extension, non-tree streams) decodes only rows [FIRST, FIRST +
 * COUNT) of the stream, in stream order, through the sidecar's chunk index, and writes only
 * those rows; it does not combine with --check-file, which compares whole files. */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "misc.h"
#include "pqh.h"
#include "vecs_io.h"

static int g_m;
static int row_cmp(const void* a, const void* b) {
    const unsigned char *x = a, *y = b;
    for (int i = 0; i < g_m; ++i) {
        if (x[i] != y[i]) return (int)x[i] - (int)y[i];
        if (!x[i]) return 0;
    }
    return 0;
}

static int full_cmp(const void* a, const void* b) { return memcmp(a, b, (size_t)g_m); }

static int usage(const char* prog) {
    fprintf(stderr, "Usage: %s <huffman output template> [--output-file <output file>]"
                    " [--check-file <pq indices file>] [--tree] [--rows <first>:<count>]\n", prog);
    return 1;
}

/* "FIRST:COUNT", both decimal, FIRST >= 0, COUNT >= 1, nothing else in the string */
static int parse_rows(const char* s, long long* first, long long* count) {
    char* end = NULL;
    if (*s < '0' || *s > '9') return 0;
    errno = 0;
    *first = strtoll(s, &end, 10);
    if (errno || *end != ':' || end[1] < '0' || end[1] > '9') return 0;
    *count = strtoll(end + 1, &end, 10);
    return !errno && *end == 0 && *count >= 1;
}

int main(int argc, const char* argv[]) {
    if (argc < 2) return usage(argv[0]);
    const char* out_file = NULL;
    const char* check = NULL;
    const char* rows = NULL;
    int tree = 0;
    for (int i = 2; i < argc; ++i) {
        if (!strcmp(argv[i], "--output-file") && i + 1 < argc) out_file = argv[++i];
        else if (!strcmp(argv[i], "--check-file") && i + 1 < argc) check = argv[++i];
        else if (!strcmp(argv[i], "--tree")) tree = 1;
        else if (!strcmp(argv[i], "--rows") && i + 1 < argc) rows = argv[++i];
        else {
            fprintf(stderr, "Unknown arg: %s\n", argv[i]);
            return 1;
        }
    }
    unsigned char* codes = NULL;
    long long n = 0;
    int m = 0;
    int rc;
    if (rows) {
        /* checked on the host, against the row count in the stream's header, before any
         * device call */
        long long first = 0, count = 0;
        if (tree || check || !parse_rows(rows, &first, &count)) return usage(argv[0]);
        char* path = concat(argv[1], "huffman_indices.bin");
        FILE* f = fopen(path, "rb");
        unsigned long long total = 0;
        const int got = f && fread(&total, 8, 1, f) == 1;
        if (f) fclose(f);
        if (!got) {
            fprintf(stderr, "huffman_decoder: cannot read %s\n", path);
            free(path);
            return 1;
        }
        free(path);
        if ((unsigned long long)first >= total || (unsigned long long)count > total - first)
            return usage(argv[0]);
        rc = pqh_decode_files_range(argv[1], first, count, &codes, &m);
        n = count;
    } else {
        /* --tree: rows come back in the stream's DFS order (huffman_decoder.c:214-247) */
        rc = tree ? pqh_decode_tree_files(argv[1], &codes, &n, &m)
                  : pqh_decode_files(argv[1], &codes, &n, &m);
    }
    if (rc) {
        fprintf(stderr, "huffman_decoder: %s\n", pqh_status_string(rc));
        return 1;
    }
    printf("Decoded\n");
    if (out_file) {
        FILE* f = fopen(out_file, "wb");
        if (!f || fwrite(codes, (size_t)m, (size_t)n, f) != (size_t)n) {
            fprintf(stderr, "cannot write %s\n", out_file);
            return 1;
        }
        fclose(f);
    }
    if (check) {
        long long cn = 0;
        int cm = 0;
        unsigned char* orig = load_vecs_light_filename(check, 1, &cn, &cm);
        if (!orig || cn != n || cm != m) {
            fprintf(stderr, "Check FAILED: shape mismatch\n");
            return 1;
        }
        g_m = m;
        /* the encoder may have sorted (strncmp order, huffman_encoder.c:316-317): compare
         * both sides as multisets under a total order */
        qsort(orig, (size_t)n, (size_t)m, full_cmp);
        qsort(codes, (size_t)n, (size_t)m, full_cmp);
        if (memcmp(orig, codes, (size_t)n * m)) {
            fprintf(stderr, "Check FAILED\n");
            return 1;
        }
        printf("Check OK!\n");
        free(orig);
        (void)row_cmp;
    }
    free(codes);
    return 0;
}
