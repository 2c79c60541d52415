// Writes the MFCC tables of one configuration (csrc/mfcc_tables.h, host code only: no HIP, no library) to stdout for
// tests/test_mfcc_tables.py: one line of key=value fields, then the blob as raw little-endian float32.
//   mfcc_tables_dump samplerate winlen winstep numcep nfilt nfft lowfreq highfreq preemph ceplifter append_energy allow_banded
// A configuration the builder refuses gives the line "rc=<code> msg=<text>" and no blob; the exit status is 0 either way.
#include <cstdio>
#include <cstdlib>

#include "../../speaker-recognition-x-vectors_amd/csrc/mfcc_tables.h"

int main(int argc, char** argv) {
    if (argc != 13) return 2;
    xvec_mfcc_cfg c = {};
    c.samplerate = atoi(argv[1]);
    c.winlen = strtof(argv[2], nullptr);
    c.winstep = strtof(argv[3], nullptr);
    c.numcep = atoi(argv[4]);
    c.nfilt = atoi(argv[5]);
    c.nfft = atoi(argv[6]);
    c.lowfreq = strtof(argv[7], nullptr);
    c.highfreq = strtof(argv[8], nullptr);
    c.preemph = strtof(argv[9], nullptr);
    c.ceplifter = atoi(argv[10]);
    c.append_energy = atoi(argv[11]);
    MfccTables t;
    ErrorText err;
    const int rc = build_mfcc_tables(c, atoi(argv[12]) != 0, t, err);
    if (rc != XVEC_OK) {
        printf("rc=%d msg=%s\n", rc, err.text);
        return 0;
    }
    using namespace fft512;
    printf("rc=0 tw_off=%d dctl_off=%d fbw_off=%d fblo_off=%d fboff_off=%d table_floats=%d f_tw1=%d f_tw2=%d f_fb=%d f_dct=%d "
           "f_band=%d f_gat=%d f_lo0=%d f_n0=%d f_lo1=%d f_n1=%d f_gat_n=%d frame_len=%d frame_step=%d log2n=%d nbins=%d fast=%d "
           "kEx=%d kPS=%d kExRow=%d kExRow0=%d kExPart=%d kMaxItems=%d kBandN=%d kBandCap=%d kBandGroups=%d kBandGat=%d blob=%zu\n",
           t.tw_off, t.dctl_off, t.fbw_off, t.fblo_off, t.fboff_off, t.table_floats, t.f_tw1, t.f_tw2, t.f_fb, t.f_dct, t.f_band,
           t.f_gat, t.f_lo0, t.f_n0, t.f_lo1, t.f_n1, t.f_gat_n, t.frame_len, t.frame_step, t.log2n, t.nbins, (int)t.fast, kEx, kPS,
           kExRow, kExRow0, kExPart, kMaxItems, kBandN, kBandCap, kBandGroups, kBandGat, t.blob.size());
    return fwrite(t.blob.data(), 4, t.blob.size(), stdout) == t.blob.size() ? 0 : 1;
}
