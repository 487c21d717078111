// Trainer scratch layout (host only, no HIP types): the one description of
// the chunk buffer s5 and the step buffer s3. Walked with a null base for the
// size and with the buffer for the pointers, so a region cannot be sized in
// one place and handed out in another (the kernels do not bounds-check).
// `Args` is TrainArgs; tools/train_layout_check.cpp walks it under ASan.
#pragma once
#include <cstddef>
#include <utility>
#include <vector>

namespace hgx_layout {

// Bump carver: every region starts 16-byte aligned relative to the base
// (covers the int2 pfo / bmeta and the int64 gacc / r0acc).
struct Carver {
  char *base = nullptr;
  size_t off = 0;
  std::vector<std::pair<size_t, size_t>> *log = nullptr;  // (offset, bytes)
  template <class T>
  void take(T *&p, size_t count) {
    off = (off + 15) / 16 * 16;
    p = base ? reinterpret_cast<T *>(base + off) : nullptr;
    if (log) log->emplace_back(off, sizeof(T) * count);
    off += sizeof(T) * count;
  }
};

// what the sizes depend on (hgx_train's launch plan)
struct Dims {
  int batch, R, dp, CB;  // CB: batches per prepared chunk
  int RPB, nblk1;        // K1: records per workgroup, workgroups per batch
  bool fused, overlap;
  int NBF, prpb;  // step: workgroups per batch, records per workgroup
  int RW, Mmax, MX, r0slots;
};

// s5. The placed buffers pfo, pidx, pcode, ptgt, pbrk twice with the overlapped
// preparation (chunk c + 1 is placed while chunk c trains): ap[1] is ap[0]
// with the second set. skey / sM by chunk parity. Returns the bytes.
template <class Args>
size_t carve_chunk(const Dims &d, Carver c, Args (&ap)[2], int *(&skey)[2], int *(&sM)[2]) {
  const size_t CB = d.CB, SB = (size_t)d.batch * d.R;
  const size_t pg = d.fused ? CB * d.NBF * d.prpb : 0;  // placed groups
  auto placed = [&](Args &a) {
    c.take(a.pfo, CB * d.Mmax);
    c.take(a.pidx, pg * d.RW);
    c.take(a.pcode, pg * d.RW);
    c.take(a.ptgt, pg * 3);
    c.take(a.pbrk, CB + 2);
  };
  Args &a = ap[0];
  // record copies padded so K1's unconditional id loads stay in bounds
  c.take(a.bidx, CB * d.batch * d.R + (size_t)d.RPB * d.R * 2 + 64);
  c.take(a.btgt, CB * d.batch * 3 + (size_t)d.RPB * 3 * 2 + 64);
  c.take(a.inv, CB * SB + (size_t)d.RPB * d.R * 2 + 64);
  c.take(a.ukey, CB * SB);
  c.take(a.uoff, CB * (SB + 1));
  c.take(a.ucount, CB);
  c.take(a.bmeta, CB);
  if (d.fused) {
    placed(a);
    c.take(a.scode, CB * SB);
    for (int i = 0; i < 2; i++) {
      c.take(skey[i], CB * d.Mmax);
      c.take(sM[i], CB);
    }
  }
  ap[1] = a;
  if (d.overlap) placed(ap[1]);
  int *slack;
  c.take(slack, d.fused ? 128 : 64);
  return c.off;
}

inline size_t r0acc_bytes(const Dims &d) {  // [3][r0slots][2][dp] int64
  return sizeof(long long) * 3 * d.r0slots * 2 * d.dp;
}

// s3: gzero (K1 partials) | gacc [3][MX][dp] int64 | shadow [3][MX][2][dp] |
// r0acc | ovf. Returns the bytes.
template <class Args>
size_t carve_step(const Dims &d, Carver c, Args &a) {
  c.take(a.gzero, (size_t)d.nblk1 * 2 * d.dp);
  c.take(a.gacc, (size_t)3 * d.MX * d.dp);
  c.take(a.shadow, (size_t)3 * d.MX * 2 * d.dp);
  c.take(a.r0acc, r0acc_bytes(d) / sizeof(long long));
  c.take(a.ovf, 16);
  return c.off;
}

}  // namespace hgx_layout
