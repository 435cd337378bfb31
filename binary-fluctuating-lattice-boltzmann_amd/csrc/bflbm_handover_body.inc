// bflbm_handover_body.inc -- the body of the hand-over kernel (schedule 3), included verbatim by k_fused_ho and by
// k_fused_ho_unit (bflbm_handover.h), so that both compile the same source and the generic kernel's instructions stay
// exactly what they were.
// In scope: TY, MODE, RAG, UNIT (compile-time; UNIT: both relaxation rates are 1.0, see d_relax_with); S, D, G, P, F, Hg,
// noise_index.
  using L = HoLayout<TY>;
  constexpr int TX = 64, NT = TX * TY;
  constexpr int LW = TX + 2, LSZ = (TX + 2) * (TY + 2);
  constexpr int NRING = 2 * (TX + 2) + 2 * TY;
  static_assert(TY >= 4 && 4 + 2 * TY <= 64 && 8 * TY <= 64, "tile shape");
  __shared__ double rp[4][2][LSZ];                     // ring of 4 planes x {rho,phi} x (TY+2)x(TX+2)
  __shared__ double gl[Q][NT];                         // g populations of the previous plane
  __shared__ double fl[Q][NT];                         // f populations of the previous plane
  __shared__ double exch[2][2][2][2][TX];              // [buf][fluid][side][0 edge row's own sum, 1 sum handed over by the row next to it][lane]
  __shared__ double accs[2][2][2][TX];                 // [stage][fluid][side][lane] z pipeline of the edge rows' own sums
  __shared__ double colacc[2][2][2][TY][6];            // [stage][fluid][side][row][kind] z pipeline of the column lanes
  __shared__ double colfin[2][2][2][TY][6];            // [buf][fluid][side][row][kind] finished column sums

  __shared__ double ntab[MODE == 1 ? BFLBM_NORMAL_TABLE_N : 4];

  int col, chunk;
  if (!fused_map(F, (int)blockIdx.x, col, chunk)) return;   // whole workgroup leaves together
  if (MODE == 1) d_load_normal_table(ntab, true);
  const int tix = col % F.ntx;
  int tiy = col / F.ntx + F.row0;
  if (tiy >= F.nty) tiy -= F.nty;
  const int x0 = tix * TX, y0 = tiy * TY;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int ty = __builtin_amdgcn_readfirstlane(tid >> 6);   // a wave is a tile row
  const int tx = lane;
  auto wrapx = [&](int v) { return v < 0 ? v + G.nx : (v >= G.nx ? v - G.nx : v); };
  auto wrapy = [&](int v) { return v < 0 ? v + G.ny : (v >= G.ny ? v - G.ny : v); };
  auto ld = [](const double* __restrict__ base, unsigned boff) { return *reinterpret_cast<const double*>(reinterpret_cast<const char*>(base) + boff); };
  auto st = [](double* __restrict__ base, unsigned boff, double v) { *reinterpret_cast<double*>(reinterpret_cast<char*>(base) + boff) = v; };

  // active extent of this tile; idle lanes / rows of a ragged tile work on a duplicate of the last active site
  const int aw = RAG ? min(TX, G.nx - x0) : TX, ah = RAG ? min(TY, G.ny - y0) : TY;
  const bool active_x = !RAG || tx < aw;
  const bool active = !RAG || (tx < aw && ty < ah);
  const int x = x0 + (RAG ? min(tx, aw - 1) : tx), y = y0 + (RAG ? min(ty, ah - 1) : ty);
  // y roles of this row in a ragged tile (wave-uniform; a full tile has exactly one per row, see row_down / row_up below)
  const bool r_bot = RAG && ty == 0, r_top = RAG && ty == ah - 1;           // edge rows: own sums -> E, travelling sum -> O
  const bool r_hdn = RAG && ah >= 2 && ty == 1;                            // its -y travelling sum completes row 0's E
  const bool r_hup = RAG && ah >= 2 && ty == ah - 2;                       // its +y travelling sum completes row ah-1's E
  const unsigned xo[3] = { (unsigned)wrapx(x - 1) * 8u, (unsigned)x * 8u, (unsigned)wrapx(x + 1) * 8u };
  const unsigned yo[3] = { (unsigned)(wrapy(y - 1) * G.pitch) * 8u, (unsigned)(y * G.pitch) * 8u, (unsigned)(wrapy(y + 1) * G.pitch) * 8u };
  const int lown = (ty + 1) * LW + (tx + 1);

  // ---- roles of this thread in the frame production
  const bool row_down = ty < 2, row_up = ty >= TY - 2;       // rows whose -y / +y travelling sums are needed
  const bool row_kind = row_down || row_up;                  // wave-uniform
  const bool edge_row = (ty == 0) || (ty == TY - 1);
  const bool is_edge = (tid < TX) || (tid >= NT - TX);       // the same as a lane predicate (keeps the producer free of uniform branches)
  const int side_y = row_down ? 0 : 1;
  const bool col_lane = (tx == 0) || (tx == aw - 1);         // aw >= 2 (host check)
  const int side_x = (tx == 0) ? 0 : 1;
  const unsigned tile_rec = (unsigned)((tiy * F.ntx + tix) * L::REC) * 8u;     // byte offset of this tile's frame in a plane
  // ---- ring site of this thread when the ring comes from frames, both fluids.  Wave 0 takes the 64 sites below
  // the tile, wave 1 the 64 above it: their two pieces (E of the neighbouring tile, O of the own one) are whole
  // 512-byte frame rows, four full lines per load.  The 4 corners and 2*TY column sites, which have up to four
  // pieces in scattered places, go to lanes of wave 2.  (Spread evenly over the four waves, every wave issued all
  // eight frame loads on parts of those rows: twice the instructions and half again the line requests.)
  const bool has_rtask = (ty < 2 && lane < aw) || (ty == 2 && lane < 4 + 2 * ah);
  int hlx = 0, hly = 0;
  if (ty == 0) { hlx = lane + 1; hly = 0; }
  else if (ty == 1) { hlx = lane + 1; hly = ah + 1; }
  else if (ty == 2 && lane < 4) { hlx = (lane & 1) ? aw + 1 : 0; hly = (lane & 2) ? ah + 1 : 0; }
  else if (ty == 2 && lane < 4 + ah) { hlx = 0; hly = lane - 4 + 1; }
  else if (ty == 2 && lane < 4 + 2 * ah) { hlx = aw + 1; hly = lane - 4 - ah + 1; }
  const int lhalo = hly * LW + hlx;
  // the frames that hold a piece of this ring site: the owner's E and the O of every other tile around it.  The site
  // is (hlx-1, hly-1) in this tile's coordinates, hence (that - offset of the tile) in the coordinates of each of the
  // 3 x 3 tiles around; when two of those are the same tile (one or two tiles per direction) they are different
  // REPRESENTATIONS of the site in that tile's frame, and at most one of them names a slot per piece.
  unsigned fo[4] = {0u, 0u, 0u, 0u};
  int nfo = 0;
  if (has_rtask) {
    const int wlast = G.nx - (F.ntx - 1) * TX, hlast = G.ny - (F.nty - 1) * TY;   // extent of the last tile column / row (TX, TY when full)
    for (int dty = -1; dty <= 1; ++dty) {
      for (int dtx = -1; dtx <= 1; ++dtx) {
        int ux = tix + dtx, uy = tiy + dty;
        ux = ux < 0 ? ux + F.ntx : (ux >= F.ntx ? ux - F.ntx : ux);
        uy = uy < 0 ? uy + F.nty : (uy >= F.nty ? uy - F.nty : uy);
        const int wu = (ux == F.ntx - 1) ? wlast : TX, hu = (uy == F.nty - 1) ? hlast : TY;
        const int lx = (hlx - 1) + (dtx < 0 ? wu : (dtx > 0 ? -aw : 0));
        const int ly = (hly - 1) + (dty < 0 ? hu : (dty > 0 ? -ah : 0));
        const int slot = ho_frame_slot<TY>(lx, ly, wu, hu);
        if (slot >= 0 && nfo < 4) { fo[nfo] = (unsigned)((uy * F.ntx + ux) * L::REC + slot) * 8u; ++nfo; }
      }
    }
  }

  const int qa = F.pa + chunk * F.cstride;
  const int qb = min(F.pb, qa + F.lz);
  auto wrapp = [&](int q) {
    if (!G.zwrap) return q;
    const int m = q % G.nzs;
    return m < 0 ? m + G.nzs : m;
  };
  // planes whose frames are complete: all three source planes collided by this workgroup
  const int fa = qa + 1, fb = qb - 2;                        // [fa, fb]

  double anb[2][2] = {{0., 0.}, {0., 0.}};                   // [fluid][stage] z pipeline of the row's travelling sum
  double aup[2][2] = {{0., 0.}, {0., 0.}};                   // RAG: the +y travelling sum runs beside the -y one (anb)

  // finish the frames of plane tpf from what the previous march position left in LDS (after a barrier)
  auto finish = [&](int tpf, int rb) {
    if (tpf < fa || tpf > fb) return;
    double* __restrict__ fp = Hg.fout + (long long)tpf * Hg.fplane;
    if (!RAG) {
      if (edge_row) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          const double e = exch[rb][k][side_y][0][lane] + exch[rb][k][side_y][1][lane];
          st(fp, tile_rec + (unsigned)(k * L::FR + (side_y ? L::ET : L::EB) + lane) * 8u, e);
        }
      }
    } else {
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        if (r_bot) st(fp, tile_rec + (unsigned)(k * L::FR + L::EB + lane) * 8u, exch[rb][k][0][0][lane] + exch[rb][k][0][1][lane]);
        if (r_top) st(fp, tile_rec + (unsigned)(k * L::FR + L::ET + lane) * 8u, exch[rb][k][1][0][lane] + exch[rb][k][1][1][lane]);
      }
    }
    if (ty == 0 && lane < 8 * TY) {
      const int k = lane / (4 * TY), rem = lane % (4 * TY), sd = rem / (2 * TY), u = rem % (2 * TY);
      const int ne = ah > 2 ? ah - 2 : 0;                      // own edge sites of the column: rows 1..ah-2
      double v = 0.; int slot = -1;
      if (u < ne) {
        const int row = u + 1;
        v = colfin[rb][k][sd][row][0] + colfin[rb][k][sd][row - 1][1] + colfin[rb][k][sd][row + 1][2];
        slot = (sd ? L::ER : L::EL) + row - 1;
      } else if (u - ne < ah + 2) {                            // ring site beside the column, rows -1..ah
        const int row = u - ne - 1;
        if (row >= 0 && row < ah) v = colfin[rb][k][sd][row][3];
        if (row - 1 >= 0 && row - 1 < ah) v += colfin[rb][k][sd][row - 1][4];
        if (row + 1 >= 0 && row + 1 < ah) v += colfin[rb][k][sd][row + 1][5];
        slot = (sd ? L::OR_ : L::OL) + row + 1;
      }
      if (slot >= 0) st(fp, tile_rec + (unsigned)(k * L::FR + slot) * 8u, v);
    }
  };

  // issue the loads of plane q: the own site's 38 populations and, when the ring of that plane comes from frames, its pieces
  // which: 0 both fluids, 1 the f half (with the frame pieces), 2 the g half; parts: 1 the own site's loads, 2 the frame pieces
  auto pull_plane = [&](int q, double (&f)[Q], double (&g)[Q], double (&hv)[2][4], const int which = 0, const int parts = 3) {
    const double* __restrict__ pl[3] = { S + (long long)wrapp(q - 1) * G.plane, S + (long long)wrapp(q) * G.plane,
                                         S + (long long)wrapp(q + 1) * G.plane };
    unsigned oo[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b2 = 0; b2 < 3; ++b2) { oo[a][b2] = yo[a] + xo[b2]; asm volatile("" : "+v"(oo[a][b2])); }
    if (parts & 1) {
#pragma unroll
      for (int i = 0; i < Q; ++i) {
        const double* __restrict__ b = pl[1 - Vel::cz[i]] + (long long)i * G.vol;
        const unsigned o = oo[1 - Vel::cy[i]][1 - Vel::cx[i]];
        if (which != 2) f[i] = ld(b, o);
        if (which != 1) g[i] = ld(b + (long long)Q * G.vol, o);
      }
    }
    if ((parts & 2) && which != 2 && Hg.use_frames && q >= fa && q <= fb && has_rtask) {
      const double* __restrict__ fp = Hg.fin + (long long)q * Hg.fplane;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        unsigned o = fo[j];
        asm volatile("" : "+v"(o));
        if (j < 2 || j < nfo) { hv[0][j] = ld(fp, o); hv[1][j] = ld(fp + L::FR, o); }
        else { hv[0][j] = 0.; hv[1][j] = 0.; }
      }
    }
  };
  double nf[Q], ng[Q], hvn[2][4];                            // the plane in flight
  // Deferred g stores (full-tile unit-rate kernel): in the steady state the outputs of fluid g wait in registers and are stored
  // by the NEXT position, as one run in front of its barrier; see the comment at the stores
  constexpr bool DEFER_G = UNIT && MODE == 0 && !RAG;
  double dg[Q];                                              // outputs of fluid g of the previous position that are not stored yet
  pull_plane(qa - 1, nf, ng, hvn);
  // The first plane is waited for here, outside the loop: the wait at the loop head is then computed from the
  // back edge alone, where the stores of the previous position are younger than every load it needs, and no
  // longer drains those stores (it was vmcnt(0), the join of this path and the back edge).
  __builtin_amdgcn_s_waitcnt(0x0F70);                        // vmcnt(0), expcnt and lgkmcnt untouched

  int it = 0;
  // One march position. The two template flags say at compile time whether this position collides a plane and whether it
  // requests the next one. The two leading positions, the steady state and the last position are separate
  // instances, so that the steady-state loop has a single path of memory operations: the compiler's wait at the
  // loop head is then the one the back edge needs -- the loads, not the 19 stores issued after them (it was
  // vmcnt(0): the join with the paths that end in loads).
  // pend_c: the previous position left its g outputs in dg; keep_c: this position leaves its own there (DEFER_G only)
  auto position = [&](const int q, auto col_c, auto ldn_c, auto pend_c, auto keep_c) {
    constexpr bool do_collide = decltype(col_c)::value, load_next = decltype(ldn_c)::value;
    constexpr bool pending = decltype(pend_c)::value, keep = decltype(keep_c)::value;
    // steady state: the own loads of the f half are spread over the relaxation of f (below)
    constexpr bool spread_f = do_collide && load_next;
    const int slot = it & 3;
    const double* __restrict__ pl[3] = { S + (long long)wrapp(q - 1) * G.plane, S + (long long)wrapp(q) * G.plane,
                                         S + (long long)wrapp(q + 1) * G.plane };
    // 1. plane q: pulled while the previous plane was collided
    double cf[Q], cg[Q], hv[2][4];
#pragma unroll
    for (int i = 0; i < Q; ++i) { cf[i] = nf[i]; cg[i] = ng[i]; }
#pragma unroll
    for (int j = 0; j < 4; ++j) { hv[0][j] = hvn[0][j]; hv[1][j] = hvn[1][j]; }
    const bool ring_from_frames = Hg.use_frames && q >= fa && q <= fb;       // uniform over the workgroup
    double zero = 0.0;
    asm volatile("" : "+v"(zero));
    auto density = [&](const double (&fs)[Q]) { double r = zero;
#pragma unroll
      for (int i = 0; i < Q; ++i) r += fs[i];
      return r; };
    if (ring_from_frames) {
      if (active) { rp[slot][0][lown] = density(cf); rp[slot][1][lown] = density(cg); }
      if (has_rtask) {
        double r0 = hv[0][0] + hv[0][1], r1 = hv[1][0] + hv[1][1];
        if (nfo > 2) { r0 += hv[0][2]; r1 += hv[1][2]; }
        if (nfo > 3) { r0 += hv[0][3]; r1 += hv[1][3]; }
        rp[slot][0][lhalo] = r0; rp[slot][1][lhalo] = r1;
      }
    } else {
      if (active) { rp[slot][0][lown] = density(cf); rp[slot][1][lown] = density(cg); }
      // pulled ring (chunk-boundary planes, first step, tile rows next to a lower last row): threads 0..nring-1 pull
      // one ring site, both fluids in one batch of 38 loads (wave-uniform base + 32-bit lane offset, like the own
      // loads); a rare path
      if (tid < (RAG ? 2 * (aw + 2) + 2 * ah : NRING)) {
        const int r = tid;
        int rx, ry;
        if (r < aw + 2) { rx = r; ry = 0; }
        else if (r < 2 * (aw + 2)) { rx = r - (aw + 2); ry = ah + 1; }
        else if (r < 2 * (aw + 2) + ah) { rx = 0; ry = r - 2 * (aw + 2) + 1; }
        else { rx = aw + 1; ry = r - 2 * (aw + 2) - ah + 1; }
        const int hx = wrapx(x0 + rx - 1), hy = wrapy(y0 + ry - 1);
        const unsigned hxo[3] = { (unsigned)wrapx(hx - 1) * 8u, (unsigned)hx * 8u, (unsigned)wrapx(hx + 1) * 8u };
        const unsigned hyo[3] = { (unsigned)(wrapy(hy - 1) * G.pitch) * 8u, (unsigned)(hy * G.pitch) * 8u, (unsigned)(wrapy(hy + 1) * G.pitch) * 8u };
        double t[2][Q];
#pragma unroll
        for (int i = 0; i < Q; ++i) {
          unsigned o = hyo[1 - Vel::cy[i]] + hxo[1 - Vel::cx[i]];
          asm volatile("" : "+v"(o));
          const double* __restrict__ b = pl[1 - Vel::cz[i]] + (long long)i * G.vol;
          t[0][i] = ld(b, o);
          t[1][i] = ld(b + (long long)Q * G.vol, o);
        }
        // all 38 requests are out before the first sum waits (left to itself the compiler issued one load, waited
        // for it, added, and went on to the next: 38 memory latencies in a row at four positions of every chunk)
        __builtin_amdgcn_sched_barrier(0);
        rp[slot][0][ry * LW + rx] = density(t[0]);
        rp[slot][1][ry * LW + rx] = density(t[1]);
      }
    }
    // The deferred outputs of fluid g of plane q-2 go out here: the loads of plane q have all arrived (the density sums above
    // consumed them), the wave issues nothing else until the f half is requested behind the barrier, and the request queue is
    // empty.  In the tail of the previous position the same stores stood between 130 VALU instructions behind the burst of g
    // requests.  512^3, interleaved processes, five each: 8660 -> 8896 MLUPS (+2.7 %; +3.4 % on the box of the scan), 256^3
    // +2.2 %; the same stores behind the barrier -3.5 %, over the hold swap +0.2 ... +0.7 %, at the top of the position +1.6 %
    // (NOTES.md section 3.1g, profiles/request_placement_ab.txt).
    if (pending) {
      double* __restrict__ Dq = D + (long long)wrapp(q - 2) * G.plane + (long long)Q * G.vol;
      unsigned oq = yo[1] + xo[1];
#pragma unroll
      for (int i = 0; i < Q; ++i) {
        if (!ho_g_deferred(i)) continue;
        asm volatile("" : "+v"(oq));                           // keeps the store in its place among the memory operations around it
        __builtin_nontemporal_store(dg[i], reinterpret_cast<double*>(reinterpret_cast<char*>(Dq + (long long)i * G.vol) + oq));
      }
    }
    __syncthreads();
    // frames of plane q-3: finished at the previous position, combined across rows now
    finish(q - 3, (it & 1) ^ 1);
    // 3. collide plane q-1
    const int pc = q - 1;
    double mg[Q], jg[3];
    if (do_collide) {
      double pg[Q];
#pragma unroll
      for (int i = 0; i < Q; ++i) pg[i] = gl[i][tid];
      d_moments(pg, mg);
      d_momentum(pg, jg);
    }
    double mf[Q], jf[3];
    if (do_collide) {
      double pfl[Q];
#pragma unroll
      for (int i = 0; i < Q; ++i) pfl[i] = fl[i][tid];
      d_moments(pfl, mf);
      d_momentum(pfl, jf);
    }
#pragma unroll
    for (int i = 0; i < Q; ++i) gl[i][tid] = cg[i];
#pragma unroll
    for (int i = 0; i < Q; ++i) fl[i][tid] = cf[i];
    // the f half of the next plane: in flight while plane q-1 is collided
    if (load_next) pull_plane(q + 1, nf, ng, hvn, 1, spread_f ? 2 : 3);
    if (do_collide) {
      const int sl[3] = { (it - 2) & 3, (it - 1) & 3, it & 3 };
      const double r = rp[sl[1]][0][lown], ph = rp[sl[1]][1][lown];
      double nb[Q], grad_rho[3], grad_phi[3];
#pragma unroll
      for (int i = 0; i < Q; ++i) nb[i] = rp[sl[1 + Vel::cz[i]]][0][lown + Vel::cy[i] * LW + Vel::cx[i]];
      d_gradient(P, nb, grad_rho);
#pragma unroll
      for (int i = 0; i < Q; ++i) nb[i] = rp[sl[1 + Vel::cz[i]]][1][lown + Vel::cy[i] * LW + Vel::cx[i]];
      d_gradient(P, nb, grad_phi);
      const int pcw = wrapp(pc);
      double fn3[3] = {0., 0., 0.}, gn3[3] = {0., 0., 0.};
      NoiseAmp NA; bflbm_rng_state rst;
      if (MODE == 1) {
        d_noise_amp(P, r, ph, r + ph, NA);
        d_noise_head(P, NA, global_site(G, x, y, pcw), noise_index, ntab, rst, fn3);
#pragma unroll
        for (int k3 = 0; k3 < 3; ++k3) gn3[k3] = -fn3[k3];
      }
      double* __restrict__ Dp = D + (long long)pcw * G.plane;
      unsigned o = yo[1] + xo[1];
      asm volatile("" : "+v"(o));
      SiteHydro Hy;
      SiteRecip R;
      d_site_recips(P, r, ph, R);
      d_hydrovars_j(P, jf, jg, r, ph, grad_rho, grad_phi, fn3, gn3, Hy, R);
      double v_b[3];
      d_barycentric(r, ph, Hy, v_b, R);
      const int tp = pc - 1;                                   // plane whose sums become complete now
      const bool tp_ok = tp >= fa && tp <= fb;
      double* __restrict__ fp = Hg.fout + (long long)tp * Hg.fplane;
      const int wb = it & 1;
      const double zn[Q] = {0.};
      // sorts the 19 outputs of one fluid by destination and advances the z pipelines (see the header comment)
      // moments -> populations from the same terms as d_populations; a group of three populations that share a
      // destination (dy,dz) is stored and folded into its x bucket right after it is formed
      auto finish_fluid = [&](const double (&mom)[Q], const int k, auto later_c) {
        PopTerms T;
        d_population_terms(mom, T);
        double* __restrict__ Dk = Dp + (long long)(k * Q) * G.vol;
        // population stores carry the non-temporal hint (round 4: +0.9 % at 512^3, +0.6 % at 256^3, +1.6 % with noise, runs agreeing to
        // 0.1 %: the written lines are not read again before the next step, the L2 keeps the neighbours' shared lines instead)
        auto put = [&](int i, double v) {
          if (decltype(later_c)::value && ho_g_deferred(i)) { dg[i] = v; return; }     // stored by the next position
          if (active) __builtin_nontemporal_store(v, reinterpret_cast<double*>(reinterpret_cast<char*>(Dk + (long long)i * G.vol) + o));
        };
        // x shifts see zeros from the idle lanes of a narrow tile (they hold a duplicate of the last site)
        auto shr = [&](double v) { return ho_shr((RAG && !active_x) ? 0.0 : v); };
        auto shl = [&](double v) { return ho_shl((RAG && !active_x) ? 0.0 : v); };
        auto diag = [&](int g, int j) {          // population j of plane g (d_populations)
          return j == 0 ? T.B[g] + T.p[g] + T.q[g] + T.r[g] : j == 1 ? T.B[g] - T.p[g] - T.q[g] + T.r[g]
               : j == 2 ? T.B[g] + T.p[g] - T.q[g] - T.r[g] : T.B[g] - T.p[g] + T.q[g] - T.r[g]; };
        const double o0 = T.rest, o1 = T.E[0] + T.O[0], o2 = T.E[0] - T.O[0];
        put(0, o0); put(1, o1); put(2, o2);
        const double x00 = o0 + shr(o1) + shl(o2);
        const double o3 = T.E[1] + T.O[1], o7 = diag(0, 0), o10 = diag(0, 3);
        put(3, o3); put(7, o7); put(10, o10);
        const double xp0 = o3 + shr(o7) + shl(o10);
        const double o4 = T.E[1] - T.O[1], o9 = diag(0, 2), o8 = diag(0, 1);
        put(4, o4); put(9, o9); put(8, o8);
        const double xm0 = o4 + shr(o9) + shl(o8);
        const double o5 = T.E[2] + T.O[2], o15 = diag(2, 0), o18 = diag(2, 2);
        put(5, o5); put(15, o15); put(18, o18);
        const double x0p = o5 + shr(o15) + shl(o18);
        const double o6 = T.E[2] - T.O[2], o17 = diag(2, 3), o16 = diag(2, 1);
        put(6, o6); put(17, o17); put(16, o16);
        const double x0m = o6 + shr(o17) + shl(o16);
        const double o11 = diag(1, 0), o12 = diag(1, 1), o13 = diag(1, 2), o14 = diag(1, 3);
        put(11, o11); put(12, o12); put(13, o13); put(14, o14);
        // what leaves the tile in x (column lanes only; side_x picks the lane's outward direction)
        const double oxp = side_x ? o15 : o18, ox0 = side_x ? o1 : o2, oxm = side_x ? o17 : o16, oyp = side_x ? o7 : o10, oym = side_x ? o9 : o8;
        if (!RAG) {
        // travelling sum towards the nearer tile edge (rows 0,1: -y; rows TY-2,TY-1: +y): contributions to
        // planes p+1, p, p-1 enter a two-stage pipeline, what leaves it is complete for plane p-1
        const double np = row_down ? o14 : o11, n0 = row_down ? xm0 : xp0, nm = row_down ? o12 : o13;
        const double fin_nb = anb[k][1] + nm;
        anb[k][1] = anb[k][0] + n0;
        anb[k][0] = np;
        double hand = fin_nb;                     // rows next to an edge row hand their sum to the edge row
        if (is_edge) {                            // (lane predicate) own sums of the edge row; its travelling sum is the ring's
          const double fin_self = accs[1][k][side_y][lane] + x0m;
          accs[1][k][side_y][lane] = accs[0][k][side_y][lane] + x00;
          accs[0][k][side_y][lane] = x0p;
          hand = fin_self;
          if (tp_ok) st(fp, tile_rec + (unsigned)(k * L::FR + (side_y ? L::OT : L::OB) + lane) * 8u, fin_nb);
        }
        if (TY == 4 || row_kind) exch[wb][k][side_y][edge_row ? 0 : 1][lane] = hand;
        } else {
        // ragged tile (1-4 rows): both travelling sums run in every row; what a row does with them is its role(s)
        const double fin_dn = anb[k][1] + o12;    // -y: lands on row ty-1 (the ring row below for row 0)
        anb[k][1] = anb[k][0] + xm0;
        anb[k][0] = o14;
        const double fin_up = aup[k][1] + o13;    // +y: lands on row ty+1 (the ring row above for row ah-1)
        aup[k][1] = aup[k][0] + xp0;
        aup[k][0] = o11;
        if (r_bot || r_top) {                     // own sums of an edge row (one pipeline: a single-row tile is both edges)
          const int sd = r_bot ? 0 : 1;
          const double fin_self = accs[1][k][sd][lane] + x0m;
          accs[1][k][sd][lane] = accs[0][k][sd][lane] + x00;
          accs[0][k][sd][lane] = x0p;
          if (r_bot) { exch[wb][k][0][0][lane] = fin_self; if (tp_ok) st(fp, tile_rec + (unsigned)(k * L::FR + L::OB + lane) * 8u, fin_dn); }
          if (r_top) { exch[wb][k][1][0][lane] = fin_self; if (tp_ok) st(fp, tile_rec + (unsigned)(k * L::FR + L::OT + lane) * 8u, fin_up); }
        }
        if (r_hdn) exch[wb][k][0][1][lane] = fin_dn;
        if (r_hup) exch[wb][k][1][1][lane] = fin_up;
        }
        if (col_lane) {
          // kinds: 0..2 sums travelling dy = 0,+1,-1 inside the column; 3..5 what leaves the tile in x with dy = 0,+1,-1
          const double vp[6] = { x0p, o11, o14, oxp, 0., 0. };
          const double v0[6] = { x00, xp0, xm0, ox0, oyp, oym };
          const double vm[6] = { x0m, o13, o12, oxm, 0., 0. };
#pragma unroll
          for (int j = 0; j < 6; ++j) {
            colfin[wb][k][side_x][ty][j] = colacc[1][k][side_x][ty][j] + vm[j];
            colacc[1][k][side_x][ty][j] = colacc[0][k][side_x][ty][j] + v0[j];
            colacc[0][k][side_x][ty][j] = vp[j];
          }
        }
      };
      // Round 3 (shader-clock stamps of the march phases): a lone wave that issues its 19 requests as one burst stands
      // at the issue for 2400 of the 18500 clocks of a position -- the burst is longer than the CU's request queue, and
      // an in-order wave cannot compute while it waits for queue space.  In the quiet kernel the 19 own loads of the f
      // half are therefore requested one every HO_SPREAD_F (28) VALU instructions of the relaxation of f; the order is
      // pinned with sched_group_barrier (the compiler hoists independent loads to the top of the block otherwise).
      // 512^3: 7817 -> 8484 and 8250 -> 8442 MLUPS on two boxes, 256^3 +2.5 %; spacings of 20 and 36 and all 38 loads
      // spread were slower than the burst (NOTES.md section 3.1f).  The noise kernel: every spacing lost with round 3's
      // generator; with round 4's (11 instructions per normal) one request every 44 instructions is +2 % at both sizes
      // (profiles/r04_noise_generator_ab.txt).
      if (spread_f) pull_plane(q + 1, nf, ng, hvn, 1, 1);
      if (MODE == 1) d_relax_generated(P, mf, r, v_b, Hy.uf, Hy.af, P.inv_tau_f_bar, fn3, NA.sr, ntab, rst, R.cs4);
      else           d_relax<false, UNIT>(P, mf, r, v_b, Hy.uf, Hy.af, P.inv_tau_f_bar, zn, R.cs4);
      if (spread_f) {
#pragma unroll
        for (int s_ = 0; s_ < Q; ++s_) {
          __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);                      // one vector-memory read,
          __builtin_amdgcn_sched_group_barrier(0x002, MODE == 1 ? HO_SPREAD_F1 : (UNIT ? (RAG ? HO_SPREAD_FU_RAG : HO_SPREAD_FU) : HO_SPREAD_F), 0);      // then this many VALU instructions
        }
      }
      finish_fluid(mf, 0, std::false_type{});
      if (load_next) pull_plane(q + 1, nf, ng, hvn, 2);       // the g half of the next plane: spreads the requests over the march position (+2.9 % at 512^3)
      if (MODE == 1) d_relax_generated(P, mg, ph, v_b, Hy.ug, Hy.ag, P.inv_tau_g_bar, gn3, NA.sp, ntab, rst, R.cs4);
      else           d_relax<false, UNIT>(P, mg, ph, v_b, Hy.ug, Hy.ag, P.inv_tau_g_bar, zn, R.cs4);
      finish_fluid(mg, 1, std::bool_constant<keep>{});
    } else if (load_next) {
      // the first two positions of a chunk collide nothing: the g half goes now, and is waited for here (as in
      // the prologue: keeps vmcnt(0) out of the loop head)
      pull_plane(q + 1, nf, ng, hvn, 2);
      __builtin_amdgcn_s_waitcnt(0x0F70);
    }
  };
  using T_ = std::true_type; using F_ = std::false_type;
  {
    int q = qa - 1;                                          // qb >= qa + 1: both leading positions request a plane
    for (int k = 0; k < 2; ++k, ++q, ++it) position(q, F_{}, T_{}, F_{}, F_{});
    if constexpr (DEFER_G) {
      // the first steady-state position finds nothing pending (its own instance, so that the loop keeps a single path of
      // memory operations); the last position of the chunk stores what the loop left and its own outputs at once
      if (q < qb) {
        position(q, T_{}, T_{}, F_{}, T_{});
        ++q; ++it;
        for (; q < qb; ++q, ++it) position(q, T_{}, T_{}, T_{}, T_{});
        position(qb, T_{}, F_{}, T_{}, F_{});
      } else {
        position(qb, T_{}, F_{}, F_{}, F_{});
      }
    } else {
      for (; q < qb; ++q, ++it) position(q, T_{}, T_{}, F_{}, F_{});
      position(qb, T_{}, F_{}, F_{}, F_{});
    }
    ++it;
  }
  // the last complete plane (qb-2) was finished at the last position; combine it across rows
  __syncthreads();
  finish(qb - 2, (it & 1) ^ 1);
