// Phases A-E of BlockLab::load + post_load for ONE component c of the block pb, behind labs_setup.hpp: they end with the fine tile of
// that component complete in lab[] behind a barrier, the caller's to consume (and to put a barrier behind, before lab[] is reused).
// The includer provides, besides what the set-up took and made,
//   nc, c                             number of components of the field, the component
//   LABS_BLOCK(slot, c)               pointer to component c of block `slot` (512 doubles)
//   LABS_CELL(slot, c, i)             cell i of it
// Grid::lab_boxes (grid.cpp) replays the block reads of phases A and B on the host: a change to them is repeated there.
    const double *__restrict__ own = LABS_BLOCK(pb, c);
    // A. centre, same-level neighbours, finer neighbours (averaged down)
    for (int e = t; e < L3; e += 256) {
      const int l[3] = {e % L - W, (e / L) % L - W, e / (L * L) - W};
      int code[3], loc[3], fl[3], q = 0;
      for (int d = 0; d < 3; ++d) {
        code[d] = l[d] < 0 ? -1 : (l[d] > 7 ? 1 : 0);
        loc[d] = l[d] - 8 * code[d];
        fl[d] = code[d] < 0 ? 8 + 2 * l[d] : (code[d] > 0 ? 2 * (l[d] - 8) : (2 * l[d]) & 7);
        if (code[d] == 0 && l[d] >= 4) q |= 1 << d;
      }
      const int icode = (code[0] + 1) + 3 * (code[1] + 1) + 9 * (code[2] + 1);
      const int n = n27[icode];
      double v = 0.0;
      if (n >= 0 && n < kNbrCoarser) v = LABS_CELL(n, c, (loc[2] * 8 + loc[1]) * 8 + loc[0]);
      else if (n == kNbrFiner && fin && fin[icode * 8 + q] >= 0) v = avg_block(LABS_BLOCK(fin[icode * 8 + q], c), fl[0], fl[1], fl[2]);
      lab[e] = v;
    }
    __syncthreads();
    if (has_coarse) {
      // B. coarse shadow tile
      for (int e = t; e < C3; e += 256) {
        const int P[3] = {e % kLabCoarse - 3, (e / kLabCoarse) % kLabCoarse - 3, e / (kLabCoarse * kLabCoarse) - 3};
        int code[3];
        for (int d = 0; d < 3; ++d) code[d] = P[d] < 0 ? -1 : (P[d] > 3 ? 1 : 0);
        const int icode = (code[0] + 1) + 3 * (code[1] + 1) + 9 * (code[2] + 1);
        const int n = n27[icode];
        double v = 0.0;
        if (icode == 13) {
          double w[8];
#pragma unroll
          for (int q = 0; q < 8; ++q) w[q] = own[((2 * P[2] + (q >> 2)) * 8 + 2 * P[1] + ((q >> 1) & 1)) * 8 + 2 * P[0] + (q & 1)];  // x fastest here
          v = avg_down8(w);
        } else if (n >= kNbrCoarser) {
          v = LABS_CELL(n - kNbrCoarser, c, ((par[2] * 4 + P[2] + 8) & 7) * 64 + ((par[1] * 4 + P[1] + 8) & 7) * 8 + ((par[0] * 4 + P[0] + 8) & 7));
        } else if (n >= 0) {
          v = avg_block(LABS_BLOCK(n, c), 2 * P[0] - 8 * code[0], 2 * P[1] - 8 * code[1], 2 * P[2] - 8 * code[2]);
        }
        Ct[e] = v;
      }
      __syncthreads();
      // C. domain faces on the coarse tile: the three ghost layers behind the face, every transverse position, from the face cell.
      //    One pass per axis does both sides: each writes ghosts of its own side and reads the face cells, which no pass writes
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        if (!((dom >> (2 * d)) & 3)) continue;
        constexpr int per_side = 3 * kLabCoarse * kLabCoarse;
        const int d1 = (d + 1) % 3, d2 = (d + 2) % 3;
        for (int i = t; i < 2 * per_side; i += 256) {
          const int side = i / per_side, j = i - side * per_side;
          if (!((dom >> (2 * d + side)) & 1)) continue;
          const int layer = j / (kLabCoarse * kLabCoarse), r = j - layer * (kLabCoarse * kLabCoarse);
          int p[3], q[3];
          p[d] = side ? 4 + layer : -1 - layer;
          q[d] = side ? 3 : 0;
          p[d1] = q[d1] = r % kLabCoarse - 3;
          p[d2] = q[d2] = r / kLabCoarse - 3;
          Ct[cix10(p[0], p[1], p[2])] = lab_bc_value(Ct[cix10(q[0], q[1], q[2])], nc, c, a.bc_comp, a.bc[d], d);
        }
        __syncthreads();
      }
      // D. ghosts behind coarser neighbours
      for (int e = t; e < L3; e += 256) {
        const int l[3] = {e % L - W, (e / L) % L - W, e / (L * L) - W};
        int code[3], X[3], bit[3], ncode = 0;
        for (int d = 0; d < 3; ++d) {
          code[d] = l[d] < 0 ? -1 : (l[d] > 7 ? 1 : 0);
          ncode += code[d] != 0;
          X[d] = l[d] >> 1;   // the coarse cell that holds this fine cell
          bit[d] = l[d] & 1;  // which of its two children along d
        }
        if (ncode == 0 || n27[(code[0] + 1) + 3 * (code[1] + 1) + 9 * (code[2] + 1)] < kNbrCoarser) continue;
        const int ax = code[0] ? 0 : (code[1] ? 1 : 2);
        const int layer = code[ax] < 0 ? -1 - l[ax] : l[ax] - 8;
        double v;
        if (ncode == 1 && layer < 2) {  // the two layers next to a face: finite-difference mode
          const int ax1 = ax == 0 ? 1 : 0, ax2 = ax == 2 ? 1 : 2;
          const int st1 = ax1 == 0 ? 1 : kLabCoarse, st2 = ax2 == 1 ? kLabCoarse : kLabCoarse * kLabCoarse;
          const double av = fd_mode_av(Ct + cix10(X[0], X[1], X[2]), X[ax1], X[ax2], st1, st2, bit[ax1], bit[ax2]);
          int cb[3] = {l[0], l[1], l[2]}, cc[3] = {l[0], l[1], l[2]};
          cb[ax] = code[ax] > 0 ? 7 : 0;
          cc[ax] = code[ax] > 0 ? 6 : 1;
          v = fd_mode_blend(av, lab[lix(cb[0], cb[1], cb[2])], lab[lix(cc[0], cc[1], cc[2])], layer);
        } else {  // deeper layers, edges and corners: TestInterp
          v = test_interp([&](int i, int j, int k) -> double { return Ct[cix10(X[0] - 1 + i, X[1] - 1 + j, X[2] - 1 + k)]; }, bit);
        }
        lab[e] = v;
      }
      __syncthreads();
    }
    // E. domain faces on the fine tile: the W ghost layers behind the face, every transverse position (the ghosts earlier passes wrote
    //    included), from the face cell; one pass per axis, both sides, as on the coarse tile
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      if (!((dom >> (2 * d)) & 3)) continue;
      constexpr int per_side = W * L * L;
      const int d1 = (d + 1) % 3, d2 = (d + 2) % 3;
      for (int i = t; i < 2 * per_side; i += 256) {
        const int side = i / per_side, j = i - side * per_side;
        if (!((dom >> (2 * d + side)) & 1)) continue;
        const int layer = j / (L * L), r = j - layer * (L * L);
        int p[3], q[3];
        p[d] = side ? 8 + layer : -1 - layer;
        q[d] = side ? 7 : 0;
        p[d1] = q[d1] = r % L - W;
        p[d2] = q[d2] = r / L - W;
        lab[lix(p[0], p[1], p[2])] = lab_bc_value(lab[lix(q[0], q[1], q[2])], nc, c, a.bc_comp, a.bc[d], d);
      }
      __syncthreads();
    }
