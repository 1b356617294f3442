// Stand-alone host program over clibd_amd/csrc/jpeg_core.h (tests/test_jpeg_cpu.py builds it with -fsanitize=address,undefined and runs
// it as a subprocess): plans and entropy-decodes every stream of a bundle from buffers of exactly the stream's and the coefficients'
// size, so a read or a write past either is an AddressSanitizer report.
//
//   jpeg_fetch_main BUNDLE [DUMP]
//
// BUNDLE: records of  u32 name length, name, u32 data length, data  (little endian).  One line per record on stdout:
//   name reason status blocks checksum        (status -1: the plan left the stream to the host)
// DUMP (optional): for every record with reason 0, i32 status, i32 blocks, then blocks * 64 int16 coefficients.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../clibd_amd/csrc/jpeg_core.h"

static bool read_u32(FILE* f, uint32_t* v) {
    unsigned char b[4];
    if (fread(b, 1, 4, f) != 4) return false;
    *v = (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24;
    return true;
}

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s BUNDLE [DUMP]\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    FILE* dump = argc > 2 ? fopen(argv[2], "wb") : nullptr;
    uint32_t nlen, dlen;
    int records = 0;
    while (read_u32(f, &nlen)) {
        std::string name(nlen, '\0');
        if (nlen && fread(&name[0], 1, nlen, f) != nlen) return 3;
        if (!read_u32(f, &dlen)) return 3;
        uint8_t* data = (uint8_t*)malloc(dlen ? dlen : 1);   // exactly the stream: no slack for an over-read to hide in
        if (dlen && fread(data, 1, dlen, f) != dlen) return 3;
        clibd_jpeg_record* plan = (clibd_jpeg_record*)malloc(sizeof(clibd_jpeg_record));
        const int reason = clibd::jpeg::jpeg_plan_stream(dlen ? data : nullptr, dlen, plan);
        int status = -1;
        long long blocks = 0;
        unsigned long long sum = 1469598103934665603ull;
        if (reason == 0) {
            blocks = plan->blocks;
            int16_t* coef = (int16_t*)calloc((size_t)blocks * 64, sizeof(int16_t));
            uint16_t zq[2][64];
            for (int t = 0; t < 2; ++t)
                for (int k = 0; k < 64; ++k) zq[t][k] = clibd::jpeg::jpeg_zq_entry(plan, t, k);
            status = clibd::jpeg::jpeg_decode_scan(data, plan->stream_len, plan, &zq[0][0], coef, blocks);
            for (long long i = 0; i < blocks * 64; ++i) sum = (sum ^ (uint16_t)coef[i]) * 1099511628211ull;
            if (dump) {
                const int32_t head[2] = {status, (int32_t)blocks};
                fwrite(head, sizeof head, 1, dump);
                fwrite(coef, sizeof(int16_t), (size_t)blocks * 64, dump);
            }
            free(coef);
        }
        printf("%s %d %d %lld %016llx\n", name.c_str(), reason, status, blocks, sum);
        free(plan);
        free(data);
        ++records;
    }
    if (dump) fclose(dump);
    fclose(f);
    fprintf(stderr, "%d records\n", records);
    return 0;
}
