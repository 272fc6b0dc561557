// riccati_latency_impl.h -- the single-QP unconstrained solve on one workgroup with fp64
// matrix cores: the reference's own call pattern (NMPC_solver.cpp:316-330 builds one QP per
// SQP iteration and calls OcpQpIpmSolver::solve on it) is a latency problem, not a
// bandwidth one.  Included by riccati_unconstr.hip inside namespace ric_f64, after
// riccati_unconstr_impl.h (its LDS image, copy and residual pass are reused).
//
// Why MFMA here and not in the batched kernels: a 16-lane QP group's 12 x 12 product is 144
// dependent-free FMAs on 12 of 16 lanes, ~13 VALU instructions per column step; on the
// batched path the chip is HBM-bound and the VALU is idle half the time anyway (DESIGN.md
// 4.2).  For ONE QP the backward sweep is a chain of 20 stages on one wave, and
// v_mfma_f64_16x16x4_f64 retires 1024 FMAs per wave instruction: the stage's seven 12 x 12
// products (13 x 13 with the vector column) become 3 MFMAs each.
//
// Tiles.  A 12 x 12 block with its vector column (13 columns: [P | p], [A | b], [H | g], ...)
// is held in the MFMA's C/D layout: lane l = (g = l >> 4, c = l & 15) register r holds
// M[g + 4 r][c] (rows >= 12, columns >= 13: zero or unused).  That layout is the B operand of
// the next product (k-block kb: lane (g, c) supplies M[4 kb + g][c] = register kb) and, for a
// symmetric M, its A operand (A[c][4 kb + g] = M[4 kb + g][c]), so P_k+1 P_k+1 B, B'(P B),
// ... chain in registers.  Transposed operands (B', A', Y') come from the LDS image, where
// blocks are column-major: lane (g, c) reads M[4 kb + g][c] at c * 12 + 4 kb + g.
//
// Backward sweep, stage k (wave 0; the four 16-lane rows compute the same column-owned
// Cholesky and solves redundantly, for free -- they issue the same instructions):
//   WB = P B,  G = R + B'WB                                      6 MFMAs (critical path)
//   W = P [A | b] + [0 | p],  [H | g] = [S | r] + B'W,  [F | f] = [Q | q] + A'W
//                                                                9 MFMAs (overlap the Cholesky)
//   L = chol(G) (column-owned, G through LDS), [Y | y] = L^-1 [H | g]
//   [P | p]_k = [F | f] - Y'[Y | y]                              3 MFMAs
// Wave 1 follows one stage behind: K = -L^-T [Y | y] (L, Y handed over in LDS), the stage
// record ([K | k] rows, P packed, p: kernels.h kWs*, the batched kernel's layout, in the HBM
// workspace) and the closed loop [Acl | bcl] = [A | b] + B [K | k] as rows in LDS.
// Forward sweep (wave 0): x_k+1 = Acl x_k + bcl; then every stage at once (one group per
// stage): u_k = K x_k + k, pi_k = P x_k + p.  Then, when asked, the residual pass.
//
// Same algorithm as riccati_step + fwd_sweep (classical Riccati, HPIPM's
// d_ocp_qp_fact_solve_kkt_unconstr), another summation order: the outputs match the batched
// kernel's to rounding (tests/test_gpu_riccati.py), not bit for bit.

constexpr int kLatThreads = 512;  // wave 0: factorization, wave 1: records, all: the passes
constexpr int kLatTile = 156;     // 13 columns x 12 rows, column-major (ld 12)
constexpr int kLatL = 90;         // packed L (78) + 1 / diag (12)
constexpr int kLatAcl = 156;      // [Acl | bcl]: 12 rows of 13

// (lat_d4, lat_mfma, lat_recip, lat_chol: mfma_lat.h, shared with ipm_latency.hip)

// LDS of the kernel (doubles): the image, the closed-loop rows, then a region the backward
// sweep uses as scratch (the G / H tile, two Y tiles and two L factors, double-buffered for
// wave 1) and the passes after it as the solution copy x, u, pi.
__host__ __device__ constexpr int lat_acl_off(int N) { return (N + 1) * kImgStage; }
__host__ __device__ constexpr int lat_scr_off(int N) { return lat_acl_off(N) + N * kLatAcl; }
__host__ __device__ constexpr int lat_scr_size(int N) {
  return (3 * N + 2) * 12 > 3 * kLatTile + 2 * kLatL ? (3 * N + 2) * 12 : 3 * kLatTile + 2 * kLatL;
}
// (+ one double: the early-factor writers' arrival counter, an int)
__host__ __device__ constexpr int lat_cnt_off(int N) { return lat_scr_off(N) + lat_scr_size(N); }
size_t lat_lds_bytes(int N) { return (size_t)(lat_cnt_off(N) + 2) * sizeof(double); }
// (one Newton step in lat_recip measured within the call pattern's noise, 99.0 / 99.8 vs
// 100.2 / 99.9 us; streaming the stages into LDS during the sweep measured slower: DESIGN.md 9.1)

// One QP (blockIdx.x) of `a` by the whole workgroup, LDS at lds_raw (lat_lds_bytes(N)).
// early_req: the request asks for the early factors (the server's per-request mailbox word;
// a launched kernel passes true and arms them by a.factors_ready alone)
template <bool RES>
__device__ __forceinline__ void lat_solve(const ProblemArgsT<double>& a, unsigned char* lds_raw,
                                          bool early_req = true) {
  double* const img = reinterpret_cast<double*>(lds_raw);
  const int N = a.N;
  double* const acl = img + lat_acl_off(N);
  double* const scr = img + lat_scr_off(N);
  double* const gh = scr;                   // G, then [H | g] (13 x 12)
  double* const ybuf = scr + kLatTile;      // [Y | y] of stages k (k & 1)
  double* const lbuf = scr + 3 * kLatTile;  // L packed + 1 / diag (k & 1)
  double* const so = scr;                   // after the sweep: x [N+1][12], u [N][12], pi [N+1][12]
  const int qp = lat_opq(blockIdx.x);
  const int tid = lat_opq(threadIdx.x);
  const int wave = tid >> 6;
  const int l = tid & 63;
  const int g = l >> 4, c = l & 15;  // tile row block, column
  const bool cv = c < 12;           // a column of a 12 x 12 block
  const bool cw = c <= 12;          // ... or the vector column
  const int cc = cv ? c : 11;       // clamped column for addressing
  auto rec = [&](int k) { return a.ws + ((size_t)k * a.batch + qp) * kWsStage; };
  // Early factors (a.factors_ready): the Riccati getters' outputs are written while wave 0 runs
  // the forward sweep (below), then the QP's host flag is set -- the caller unpacks P and K
  // under the kernel's tail (the forward sweep, u, pi, the residual pass).
  const bool early = a.factors_ready != nullptr && early_req;
  const int egrp = (tid >> 4) - 4;  // 16-lane group among waves 1.. (0 = wave 1's first)
  int* const ecnt = reinterpret_cast<int*>(img + lat_cnt_off(N));
  if (tid == 0) *ecnt = 0;  // (the copy's barrier orders it before any arrival)
  tstamp(16);
  lds_copy_range(a, img, qp, 0, (N + 1) * kImgStage, tid, kLdsCopyThreads);  // (lds_copy_qp)
  tstamp(14);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  tstamp(15);

  // ---------------- backward sweep ----------------
  lat_d4 Pt;  // [P | p]_k+1 (wave 0)
  if (wave == 0) {
    const double* sl = img + N * kImgStage;
    sfor<0, 4>([&](auto rr) {
      constexpr int R = decltype(rr)::value;
      const int row = g + 4 * R < 12 ? g + 4 * R : 11;
      const double v = sl[cv ? kImgQ + c * 12 + row : kImgq + row];
      Pt[R] = (g + 4 * R < 12 && cw) ? v : 0.0;
    });
    // terminal record: P_N packed, p_N
    double* rn = rec(N);
    sfor<0, 3>([&](auto rr) {
      constexpr int R = decltype(rr)::value;
      const int row = g + 4 * R;
      if (cv && row >= c) rn[kWsP + packed_col(c) + row - c] = Pt[R];
      if (c == 12) rn[kWsp + row] = Pt[R];
    });
  }
  // stage j's second half (wave 1): K = -L^-T [Y | y], the record, [Acl | bcl]
  auto finish_stage = [&](int j) {
    const double* lb = lbuf + (j & 1) * kLatL;
    const double* yb = ybuf + (j & 1) * kLatTile;
    double Lc[12], Yc[12], Kc[12];
    load_packed_lcol(lb, cc, Lc);  // (strictly lower part: the solve uses 1 / diag)
    const double rs = lb[78 + cc];
    sfor<0, 12>([&](auto i) { Yc[decltype(i)::value] = cw ? yb[c * 12 + decltype(i)::value] : 0.0; });
    trsv_upper_t_neg_axpy(Lc, rs, Yc, Kc);  // lane c < 12: K[:, c]; lane 12: k
    double* rj = rec(j);
    if (l < 16 && cw)
      sfor<0, 12>([&](auto i) { rj[kWsK + decltype(i)::value * kWsRow + c] = Kc[decltype(i)::value]; });
    // [Acl | bcl][:, c] = [A | b][:, c] + B [K | k][:, c]
    const double* sl = img + j * kImgStage;
    double Ac[12], Bc[12];
    sfor<0, 12>([&](auto i) {
      constexpr int I = decltype(i)::value;
      const double av = sl[cv ? kImgA + c * 12 + I : kImgb + I];
      Ac[I] = cw ? av : 0.0;
      const double bv = sl[kImgB + cc * 12 + I];
      Bc[I] = cv ? bv : 0.0;
    });
    sfor<0, 12>([&](auto m) {
      constexpr int M = decltype(m)::value;
      fma_bcast_src<M>(Ac, Bc, Kc[M]);
    });
    if (l < 16 && cw)
      sfor<0, 12>([&](auto i) { acl[j * kLatAcl + decltype(i)::value * 13 + c] = Ac[decltype(i)::value]; });
  };
#pragma unroll 1
  for (int k = N - 1; k >= 0; --k) {
    if (wave == 0) {
      tstamp(0);
      const double* sl = img + k * kImgStage;
      double bo[3], ao[3];
      sfor<0, 3>([&](auto kb) {
        constexpr int KB = decltype(kb)::value;
        const int m = 4 * KB + g;
        const double bv = sl[kImgB + cc * 12 + m];
        bo[KB] = cv ? bv : 0.0;  // B[m][c]: B operand of P B; A operand (B') of B'WB, B'W
        const double av = sl[cv ? kImgA + c * 12 + m : kImgb + m];
        ao[KB] = cw ? av : 0.0;  // [A | b][m][c]: B operand of P [A | b]; A operand (A') of A'W
      });
      lat_d4 Rt, St, Qt;
      sfor<0, 4>([&](auto rr) {
        constexpr int R = decltype(rr)::value;
        const bool rok = g + 4 * R < 12;
        const int row = rok ? g + 4 * R : 11;
        const double rv = sl[kImgR + cc * 12 + row];
        const double sv = sl[cv ? kImgS + c * 12 + row : kImgr + row];
        const double qv = sl[cv ? kImgQ + c * 12 + row : kImgq + row];
        Rt[R] = rok && cv ? rv : 0.0;
        St[R] = rok && cw ? sv : 0.0;
        Qt[R] = rok && cw ? qv : 0.0;
      });
      // WB = P B; G = R + B'WB (the critical path)
      lat_d4 WB = {0.0, 0.0, 0.0, 0.0};
      sfor<0, 3>([&](auto kb) { WB = lat_mfma(Pt[decltype(kb)::value], bo[decltype(kb)::value], WB); });
      lat_d4 Gt = Rt;
      sfor<0, 3>([&](auto kb) { Gt = lat_mfma(bo[decltype(kb)::value], WB[decltype(kb)::value], Gt); });
      // W = P [A | b] + [0 | p]; [H | g] = [S | r] + B'W; [F | f] = [Q | q] + A'W: issued one
      // per pivot inside the Cholesky below (W0 W1 W2 H0 F0 H1 F1 H2 F2)
      lat_d4 Wt;
      sfor<0, 4>([&](auto rr) { Wt[decltype(rr)::value] = c == 12 ? Pt[decltype(rr)::value] : 0.0; });
      lat_d4 Ht = St, Ft = Qt;
      auto wh = [&](auto kk) {
        constexpr int K = decltype(kk)::value;
        if constexpr (K < 3) {
          Wt = lat_mfma(Pt[K], ao[K], Wt);
        } else if constexpr (K < 9) {
          constexpr int KB = (K - 3) / 2;
          if constexpr ((K - 3) % 2 == 0) {
            Ht = lat_mfma(bo[KB], Wt[KB], Ht);
          } else {
            Ft = lat_mfma(ao[KB], Wt[KB], Ft);
          }
        }
      };
      tstamp(1);
      // G to column-owned registers through LDS, Cholesky
      lds_wave_fence();
      sfor<0, 3>([&](auto rr) {
        constexpr int R = decltype(rr)::value;
        if (cv) gh[c * 12 + g + 4 * R] = Gt[R];
      });
      lds_wave_fence();
      double Gc[12], Lc[12], rs;
      sfor<0, 12>([&](auto i) {
        const double v = gh[cc * 12 + decltype(i)::value];
        Gc[decltype(i)::value] = cv ? v : 0.0;
      });
      lat_chol(Gc, c, a.reg, Lc, rs, wh);
      tstamp(3);
      // [Y | y] = L^-1 [H | g]
      lds_wave_fence();
      sfor<0, 3>([&](auto rr) {
        constexpr int R = decltype(rr)::value;
        if (cw) gh[c * 12 + g + 4 * R] = Ht[R];
      });
      lds_wave_fence();
      double Yc[12];
      sfor<0, 12>([&](auto i) {
        const double v = gh[(cw ? c : 12) * 12 + decltype(i)::value];
        Yc[decltype(i)::value] = cw ? v : 0.0;
      });
      trsv_lower(Lc, rs, Yc);
      tstamp(7);
      // hand L and [Y | y] to wave 1 (and to the Y'Y operands)
      double* yb = ybuf + (k & 1) * kLatTile;
      double* lb = lbuf + (k & 1) * kLatL;
      if (l < 16) {
        if (cw) store12(yb + c * 12, Yc);
        if (cv) {
          store_packed_col(lb, c, Lc);
          lb[78 + c] = rs;
        }
      }
      lds_wave_fence();
      // [P | p]_k = [F | f] - Y'[Y | y]
      lat_d4 Pn = Ft;
      sfor<0, 3>([&](auto kb) {
        constexpr int KB = decltype(kb)::value;
        const double yv = yb[(cw ? c : 12) * 12 + 4 * KB + g];
        const double yB = cw ? yv : 0.0;  // [Y | y][m][c]
        const double yA = cv ? -yv : 0.0;  // -(Y')[c][m]
        Pn = lat_mfma(yA, yB, Pn);
      });
      // exactly symmetric from its lower triangle, as the batched kernels (solve_qp) and for
      // their reason: the antisymmetric rounding of A'(P A) would grow by rho(A)^2 per stage.
      // Through the G / H tile, which is free here; the vector column stays as it is.
      lds_wave_fence();
      sfor<0, 3>([&](auto rr) {
        constexpr int R = decltype(rr)::value;
        if (cv && g + 4 * R >= c) gh[c * 12 + g + 4 * R] = Pn[R];
      });
      lds_wave_fence();
      sfor<0, 3>([&](auto rr) {
        constexpr int R = decltype(rr)::value;
        const double v = gh[(g + 4 * R) * 12 + cc];  // P[c][g + 4 R], of the lower triangle where row < c
        if (cv && g + 4 * R < c) Pn[R] = v;
      });
      lds_wave_fence();
      Pt = Pn;
      tstamp(9);
      // record: P packed, p (the batched kernel's layout)
      double* rk = rec(k);
      sfor<0, 3>([&](auto rr) {
        constexpr int R = decltype(rr)::value;
        const int row = g + 4 * R;
        if (cv && row >= c) rk[kWsP + packed_col(c) + row - c] = Pt[R];
        if (c == 12) rk[kWsp + row] = Pt[R];
      });
    } else if (wave == 1 && k < N - 1) {
      finish_stage(k + 1);
    }
    __syncthreads();
  }
  if (wave == 1) finish_stage(0);
  __syncthreads();  // records and closed-loop rows complete; the scratch region is free
  tstamp(12);

  // ---- the factors' rows, by waves 1.. while wave 0 runs the forward sweep: items P_0..P_N,
  // then [K | k]_0..N-1, at most two per 16-lane group (lane = row; lanes 12..15 repeat row
  // 11).  Each is written to the Riccati getters' outputs (P symmetric: row = column; K is
  // nu x nx column-major, so a row is 12 strided stores, each contiguous across the group's
  // lanes) and kept for u_k = K x_k + k, pi_k = P x_k + p after the sweep. ----
  constexpr int kItemGroups = kLatThreads / 16 - 4;  // waves 1..7
  static_assert(2 * kItemGroups >= 2 * 20 + 1, "two items per group cover N <= 20 (lat_fits)");
  const int lane = l & 15, row = lane < 12 ? lane : 11;
  double V[2][12], vv[2];
  if (wave >= 1) {
    sfor<0, 2>([&](auto ss) {
      constexpr int S = decltype(ss)::value;
      const int it = egrp + S * kItemGroups;
      if (it <= N) {
        const double* rk = rec(it);
        load_packed_sym(rk + kWsP, row, V[S]);
        vv[S] = rk[kWsp + row];
        if (a.P && lane < 12) store12(a.P + ((size_t)qp * (N + 1) + it) * 144 + (size_t)lane * 12, V[S]);
        if (a.p && lane < 12) a.p[((size_t)qp * (N + 1) + it) * 12 + lane] = vv[S];
      } else if (it <= 2 * N) {
        const int k = it - N - 1;
        const double* rk = rec(k);
        sfor<0, 12>([&](auto j) { V[S][decltype(j)::value] = rk[kWsK + row * kWsRow + decltype(j)::value]; });
        vv[S] = rk[kWsK + row * kWsRow + 12];
        if (a.k && lane < 12) a.k[((size_t)qp * N + k) * 12 + lane] = vv[S];
        if (a.K && lane < 12) {
          double* ko = a.K + ((size_t)qp * N + k) * 144 + lane;
          sfor<0, 12>([&](auto j) { ko[decltype(j)::value * 12] = V[S][decltype(j)::value]; });
        }
      }
    });
    if (early) {
      // each writer wave waits for its stores to reach the cache, then arrives; the last
      // arrival writes the cache back to host memory and sets the QP's host flag (the system-
      // scope release store: one L2 write-back for all waves, then a vector store)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if ((l & 63) == 0 && atomicAdd(ecnt, 1) == kLatThreads / 64 - 2)
        __hip_atomic_store(a.factors_ready + qp, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }

  // ---------------- forward sweep: x_k+1 = Acl x_k + bcl (wave 0, matrix cores) ----------------
  // x rides in column 0 of an MFMA tile: the product's C/D registers are the next product's B
  // operand (lane (g, c) register kb = D[4 kb + g][c]), so the chain is three MFMAs per stage.
  // Columns 1.. of x, bcl and rows 12.. of Acl are zero, so D keeps them zero.
  if (wave == 0) {
    double* xo = a.x + (size_t)qp * (N + 1) * 12;
    lat_d4 X;
    sfor<0, 4>([&](auto rr) {
      constexpr int R = decltype(rr)::value;
      const int row = g + 4 * R < 12 ? g + 4 * R : 11;
      const double v = a.x0[(size_t)qp * 12 + row];
      X[R] = (c == 0 && g + 4 * R < 12) ? v : 0.0;
    });
    double Ao[3], An[3];
    lat_d4 Ct, Cn;
    // stage k's A operand (lane (g, c), k-block kb: Acl[c][4 kb + g]) and C (bcl in column 0)
    auto load_ops = [&](int k, double (&A3)[3], lat_d4& C4) {
      const double* r = acl + k * kLatAcl + cc * 13;
      sfor<0, 3>([&](auto kb) {
        const double v = r[4 * decltype(kb)::value + g];
        A3[decltype(kb)::value] = cv ? v : 0.0;
      });
      const double* bc = acl + k * kLatAcl + 12;
      sfor<0, 4>([&](auto rr) {
        constexpr int R = decltype(rr)::value;
        const int row = g + 4 * R < 12 ? g + 4 * R : 11;
        const double v = bc[row * 13];
        C4[R] = (c == 0 && g + 4 * R < 12) ? v : 0.0;
      });
    };
    load_ops(0, Ao, Ct);
#pragma unroll 1
    for (int k = 0; k < N; ++k) {
      if (c == 0)
        sfor<0, 3>([&](auto rr) {
          constexpr int R = decltype(rr)::value;
          so[k * 12 + g + 4 * R] = X[R];
          xo[(size_t)k * 12 + g + 4 * R] = X[R];
        });
      if (k + 1 < N) load_ops(k + 1, An, Cn);
      lat_d4 D = Ct;
      sfor<0, 3>([&](auto kb) { D = lat_mfma(Ao[decltype(kb)::value], X[decltype(kb)::value], D); });
      X = D;
      sfor<0, 3>([&](auto kb) { Ao[decltype(kb)::value] = An[decltype(kb)::value]; });
      Ct = Cn;
    }
    if (c == 0)
      sfor<0, 3>([&](auto rr) {
        constexpr int R = decltype(rr)::value;
        so[N * 12 + g + 4 * R] = X[R];
        xo[(size_t)N * 12 + g + 4 * R] = X[R];
      });
  }
  __syncthreads();
  tstamp(13);

  // ---------------- every stage at once: u_k = K x_k + k, pi_k = P x_k + p ----------------
  bool bad = false;
  if (wave >= 1) {
    sfor<0, 2>([&](auto ss) {
      constexpr int S = decltype(ss)::value;
      const int it = egrp + S * kItemGroups;
      if (it <= 2 * N) {
        const int k = it <= N ? it : it - N - 1;
        const double xk = lane < 12 ? so[k * 12 + lane] : 0.0;
        const double v = dot_bcast(V[S], xk, vv[S]);
        if (lane < 12) {
          if (it <= N) {
            so[(2 * N + 1) * 12 + k * 12 + lane] = v;
            a.pi[((size_t)qp * (N + 1) + k) * 12 + lane] = v;
            bad |= !(xk == xk);
          } else {
            so[(N + 1) * 12 + k * 12 + lane] = v;
            a.u[((size_t)qp * N + k) * 12 + lane] = v;
            bad |= !(v == v);
          }
        }
      }
    });
  }
  const int any_bad = __syncthreads_or(bad);
  tstamp(17);
  if (tid == 0) {
    if (a.status) a.status[qp] = any_bad ? 3 : 0;
    if (a.iter) a.iter[qp] = 0;
  }
  if constexpr (RES) {
    ResLds acc{};
    acc.img = img;
    acc.so = so;
    acc.N = N;
    unconstr_residuals_body<ResLds, 12>(a, acc, qp, tid);
  }
  tstamp(18);
}

template <bool RES>
__global__ void __launch_bounds__(kLatThreads, 1) riccati_latency_kernel(ProblemArgsT<double> a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  lat_solve<RES>(a, lds_raw);
}

// The same solve as a resident server for the one-QP host call (capi_host.hip, the
// reference's call pattern): one workgroup stays on its CU and polls the mailbox in mapped
// host memory, so a call costs no launch, no dispatch and no completion signal -- the host
// posts a request number, the kernel solves the QP from the (fixed) staging buffer `a` points
// into and writes the number back.  It leaves on `quit`, after idle_ticks (wall clock) with
// no request, or after the first answer once life_ticks have passed since its launch (a
// bound on how long anything queued behind it on a shared hardware queue can wait), recording
// its epoch in `exited`; the host relaunches it then.
template <bool RES>
__global__ void __launch_bounds__(kLatThreads, 1)
    riccati_latency_server_kernel(ProblemArgsT<double> a, LatMailbox* mb, int epoch, int last_done,
                                  long long idle_ticks, long long life_ticks) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  int* const req = reinterpret_cast<int*>(reinterpret_cast<double*>(lds_raw) + lat_cnt_off(a.N)) + 1;
  long long t0 = wall_clock64();
  const long long t_launch = t0;
  for (;;) {
    if (threadIdx.x == 0) {
      // seq and quit in one 8-byte read of the mailbox, four reads in flight (one issued
      // every ~0.2 us, each checked a PCIe round trip later): a post is seen about one round
      // trip after it lands
      auto poll = [&]() {
        return __hip_atomic_load(reinterpret_cast<unsigned long long*>(mb), __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_SYSTEM);
      };
      int r = -1;
      unsigned long long arm = 0;
      auto seen = [&](unsigned long long v) {  // true: leave the poll (r = the request, or -1)
        if ((int)(unsigned)v != last_done) {
          r = (int)(unsigned)v;
          arm = (v >> 32) & kLatArm;
          return true;
        }
        return ((v >> 32) & kLatQuit) != 0 || wall_clock64() - t0 > idle_ticks;
      };
      // past its lifetime (checked after an answer, by thread 0 alone: the decision reaches
      // every wave through *req) the server leaves instead of polling
      const bool expired = t0 != t_launch && t0 - t_launch > life_ticks;
      unsigned long long p0 = expired ? ((unsigned long long)kLatQuit << 32) | (unsigned)last_done : poll();
      __builtin_amdgcn_s_sleep(8);
      unsigned long long p1 = poll();
      __builtin_amdgcn_s_sleep(8);
      unsigned long long p2 = poll();
      __builtin_amdgcn_s_sleep(8);
      unsigned long long p3 = poll();
      for (;;) {
        if (seen(p0)) break;
        p0 = poll();
        __builtin_amdgcn_s_sleep(8);
        if (seen(p1)) break;
        p1 = poll();
        __builtin_amdgcn_s_sleep(8);
        if (seen(p2)) break;
        p2 = poll();
        __builtin_amdgcn_s_sleep(8);
        if (seen(p3)) break;
        p3 = poll();
        __builtin_amdgcn_s_sleep(8);
      }
      // the request's inputs: drop any cached copy of the mapped staging buffer
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
      *req = r;
      // per-request early-factor switch, posted with the request number (the flags pointer is
      // fixed for the server's life, so alternating callback / plain calls do not relaunch it)
      req[1] = arm ? 1 : 0;
    }
    __syncthreads();
    const int r = *req;
    if (r < 0) break;
    lat_solve<RES>(a, lds_raw, req[1] != 0);
    // every wave's outputs in the cache, then one write-back to host memory with the answer
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(&mb->done, r, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    last_done = r;
    t0 = wall_clock64();
  }
  if (threadIdx.x == 0) __hip_atomic_store(&mb->exited, epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// the latency kernel's LDS fits the device (N <= 20 at fp64)
bool lat_fits(int N) { return lat_lds_bytes(N) + kLdsResStatic <= kLdsBytesMax; }

// (LatMailbox, the server's launch and its eligibility: kernels.h)
