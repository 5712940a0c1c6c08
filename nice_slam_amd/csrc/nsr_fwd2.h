// nsr_fwd2.h -- the forward of a differentiated render call as three launches (second generation), included by nsr_kernels.h.
//
// render_fwd_kernel (nsr_kernels.h) evaluates the decoders of a stage one after the other inside every block: each block
// stages up to three operand streams (61-82 KB each) for twelve tiles of work, with two block barriers per decoder -- a wave
// timeline of the colour stage at 1000 rays (profiles/r03_fwd_timeline.txt) shows 40 us of decoder work (the matrix-core
// bound) in 87 us: the rest is staging, the skew of twelve waves meeting at six barriers, and a serial prologue / epilogue.
// When the call saves activations for the split backward (nsr_render_args.acts + zvals) the forward takes the split
// backward's shape instead:
//   fwd_sample_kernel        one wave per ray (lane = sample): sample placement (Renderer.py:88-170) and the fp64 sample
//                            positions (Renderer.py:172-174) -> zvals, pd, pf: sample_candidate, stable_rank and sample_pos
//                            (nsr_kernels.h), the functions compute_z and render_fwd_kernel place their samples with.
//   render_fwd_pass_kernel   grid = (blocks, decoder passes): a block stages ONE decoder's stream once and its waves walk the
//                            16-point tiles of the pass independently -- no barrier after the staging.  Feature gather,
//                            decoder (mlp_xyz_fwd / mlp_nox_fwd with the activation sink), the decoder's output per sample:
//                            occupancy parts into the (still unused) d raw array of the workspace, colours into `raw`.
//   fwd_composite_kernel     one wave per ray: occupancy = fine + middle (decoder.py:333,341), bound override
//                            (Renderer.py:57), raw, compositor (common.py:231-244), depth / variance / colour (composite) and the
//                            fused mapping loss (mapping_loss_ray, Mapper.py:487-493) like the second half of render_fwd_kernel,
//                            then d raw for the split backward: comp_docc, the function comp_bwd_kernel runs.
// Small batches gain twice: the decoder passes of the tracker's 200 rays run side by side on different CUs instead of one
// after the other in 50 blocks.
#pragma once

namespace nsr {

// ------------------------------------------------------------------------------------------------
// (1) sample placement + positions, one wave per ray
// ------------------------------------------------------------------------------------------------
NSR_KERNEL void fwd_sample_kernel(const RenderParams P) {
    double *zs = reinterpret_cast<double *>(lds_base());             // [waves][64] rank-sort scratch
    const int lane = tid() & 63, wave = tid() >> 6, nw = nthreads() >> 6;
    const long long ray = (long long)bid_x() * nw + wave;
    const int S = P.S;
    double *zw = zs + wave * 64;
    if (ray >= P.n_rays) return;                                     // whole wave (no block barrier below)
    // (rays the pre-filter removed are placed too: a tile that straddles a removed and a kept ray is evaluated as a whole)
    const bool act = lane < S;
    const int k = act ? lane : 0;
    const bool guided = depth_guided(P);
    double z = sample_candidate(P, ray, k, guided);
    if (P.n_surface > 0 && guided) {
        if (act) zw[lane] = z;
        wave_fence();
        const int rank = stable_rank(zw, S, k, z);
        wave_fence();
        if (act) zw[rank] = z;
        wave_fence();
        z = act ? zw[lane] : 0.0;
    }
    if (!act) return;
    const long long gq = ray * S + lane;
    P.zvals[gq] = z;
    store_pos(P, gq, sample_pos(P, ray, z), z);
}

// ------------------------------------------------------------------------------------------------
// (2) one decoder pass over the tiles of the sample list
// ------------------------------------------------------------------------------------------------
// Blocks [pass_beg[p], pass_beg[p + 1]) of the launch belong to decoder pass p (more of them for the fine decoder: 288 instead
// of 240 MFMAs per tile and two feature gathers); block i of the n of a pass owns the contiguous tile range
// [T i / n, T (i + 1) / n) and its waves draw tiles from it through an LDS counter -- no rounds, a wave that gets a cheap
// tile (rays that left the bound) simply takes the next one.
template <int KIND, bool SAVE>
NSR_DEV void fwd_pass(const RenderParams &P, int bi, int nbp) {
    float *aux = reinterpret_cast<float *>(lds_base());
    float *wl = aux + AUX_FLOATS;
    int *cnt = reinterpret_cast<int *>(wl + packed_total(KIND));
    const int lane0 = tid() & 63, wave = tid() >> 6;
    const DecDev &D = P.dec[KIND];
    const Dbg dbg{P.dbg ? P.dbg + ((long long)bid_x() * 12 + wave) * 64 : nullptr};
    dbg.stamp(0);
    load_aux<KIND>(aux, D.packed);
    copy_f4_dma<packed_total(KIND) / 4>(wl, D.packed + AUX_FLOATS);      // (global -> LDS DMA, like the dX kernel's stream: round 6)
    if (tid() == 0) cnt[0] = 0;
    dma_wait<0>();
    block_sync();
    dbg.stamp(1);
    const long long ntiles = (P.n_points_total + kTile - 1) / kTile;
    const long long t0 = ntiles * bi / nbp, t1 = ntiles * (bi + 1) / nbp;
    for (;;) {
        int take = 0;
        if (lane0 == 0) take = atomic_fetch_add_lds_i(cnt, 1);
        const long long tile = t0 + shfl_i(take, 0);
        if (tile >= t1) break;
        if (!tile_live(P, tile)) continue;                           // every ray of the tile was removed by the pre-filter
        loop_fence();
        const int lane = opaque_i(lane0), pt = lane & 15, g = lane >> 4;      // (lane-dependent addresses formed per tile: see opaque_i)
        const long long gp = tile * kTile + pt;
        const bool active = gp < P.n_points_total;
        const double *pp = P.pd + (active ? gp : 0) * 4;
        const double px = pp[0], py = pp[1], pz = pp[2];
        dbg.stamp(2);
        const long long sp = (SAVE && active) ? gp : -1;
        float *scr = P.draw + gp * 4;                                // per-sample scratch of the passes (d raw comes later)
        if (KIND == NSR_COARSE) {
            const Lvl L = make_level(P.grid[NSR_COARSE], px, py, pz);
            const Act<2> c = gather_feat(P.grid[NSR_COARSE], L, g);
            float o[1];
            const ActSink sk = act_sink(P, 0, sp, g);
            mlp_nox_fwd<SAVE>(wl, aux, c, lane, o, &sk);
            if (active && g == 0) scr[0] = o[0];
        } else {
            const float fx = (float)px, fy = (float)py, fz = (float)pz;     // decoder.py:189
            if (KIND == NSR_MIDDLE) {
                const Lvl Lm = make_level(P.grid[NSR_MIDDLE], px, py, pz);
                const Act<2> cm = gather_feat(P.grid[NSR_MIDDLE], Lm, g);
                float om[1];
                const ActSink sk = act_sink(P, 0, sp, g);
                mlp_xyz_fwd<NSR_MIDDLE, SAVE>(wl, aux, fx, fy, fz, cm, lane, om, &sk);
                if (active && g == 0) scr[0] = om[0];
            } else if (KIND == NSR_FINE) {
                const Lvl Lf = make_level(P.grid[NSR_FINE], px, py, pz);
                const Act<2> cf = gather_feat(P.grid[NSR_FINE], Lf, g);
                const Lvl Lm = make_level(P.grid[NSR_MIDDLE], px, py, pz);
                const Act<2> cm = gather_feat(P.grid[NSR_MIDDLE], Lm, g);
                Act<4> cc;
                cc.t[0] = cf.t[0]; cc.t[1] = cf.t[1]; cc.t[2] = cm.t[0]; cc.t[3] = cm.t[1];    // decoder.py:182-187
                float of[1];
                const ActSink sk = act_sink(P, 1, sp, g);
                mlp_xyz_fwd<NSR_FINE, SAVE>(wl, aux, fx, fy, fz, cc, lane, of, &sk);
                if (active && g == 0) scr[1] = of[0];
            } else {
                const Lvl Lc = make_level(P.grid[NSR_COLOR], px, py, pz);
                const Act<2> ccol = gather_feat(P.grid[NSR_COLOR], Lc, g);
                float oc[4];
                const ActSink sk = act_sink(P, 2, sp, g);
                mlp_xyz_fwd<NSR_COLOR, SAVE>(wl, aux, fx, fy, fz, ccol, lane, oc, &sk);
                if (active && g == 0) { float *rw = P.raw + gp * 4; rw[0] = oc[0]; rw[1] = oc[1]; rw[2] = oc[2]; }
            }
        }
        dbg.stamp(3);
    }
    dbg.stamp(9);
}

template <int STAGE, bool SAVE>
NSR_KERNEL NSR_BOUNDS(768) void render_fwd_pass_kernel(const RenderParams P) {
    const int b = bid_x();
    if (STAGE == NSR_STAGE_COARSE) {
        fwd_pass<NSR_COARSE, SAVE>(P, b, nblk_x());
    } else {
        if (b < P.pass_beg[1]) fwd_pass<NSR_MIDDLE, SAVE>(P, b, P.pass_beg[1]);
        else if (b < P.pass_beg[2]) { if (STAGE >= NSR_STAGE_FINE) fwd_pass<NSR_FINE, SAVE>(P, b - P.pass_beg[1], P.pass_beg[2] - P.pass_beg[1]); }
        else { if (STAGE == NSR_STAGE_COLOR) fwd_pass<NSR_COLOR, SAVE>(P, b - P.pass_beg[2], P.pass_beg[3] - P.pass_beg[2]); }
    }
}

// ------------------------------------------------------------------------------------------------
// (3) raw, compositor, outputs, fused loss: one wave per ray
// ------------------------------------------------------------------------------------------------
template <int STAGE>
NSR_KERNEL void fwd_composite_kernel(const RenderParams P) {
    double *red = reinterpret_cast<double *>(lds_base());            // [waves] loss terms of the block
    const int lane = tid() & 63, wave = tid() >> 6, nw = nthreads() >> 6;
    const long long rayq = (long long)bid_x() * nw + wave;
    const int S = P.S;
    double lterm = 0.0;
    if (rayq < P.n_rays && !ray_live(P, rayq)) {                     // removed by the pre-filter: no sample was evaluated
        if (lane == 0) {
            P.depth[rayq] = 0.0; P.var[rayq] = 0.0;
            P.rgb[rayq * 3 + 0] = 0.f; P.rgb[rayq * 3 + 1] = 0.f; P.rgb[rayq * 3 + 2] = 0.f;
            if (P.loss && P.dl_depth) P.dl_depth[rayq] = 0.0;
            if (P.loss && P.dl_rgb) { P.dl_rgb[rayq * 3 + 0] = 0.f; P.dl_rgb[rayq * 3 + 1] = 0.f; P.dl_rgb[rayq * 3 + 2] = 0.f; }
        }
        // its samples inside a tile shared with a kept ray carry no gradient
        if (P.loss && P.dl_depth && lane < S) st4(P.draw + (rayq * S + lane) * 4, F4{0.f, 0.f, 0.f, 0.f});
    } else if (rayq < P.n_rays) {
        const bool act = lane < S;
        const long long gq = rayq * S + (act ? lane : 0);
        // the loss epilogue's inputs are requested HERE, with the sample data: behind the stores below the compiler may not move them
        // (the pointers could alias), and they were a second memory round trip in an 8 us kernel
        const bool kp = !P.loss || !P.keep || P.keep[rayq];
        const float gd = (P.loss && P.loss_depth) ? P.loss_depth[rayq] : 0.f;
        float gtc[3] = {0.f, 0.f, 0.f};
        if (P.loss && STAGE == NSR_STAGE_COLOR && P.gt_color) { gtc[0] = P.gt_color[rayq * 3 + 0]; gtc[1] = P.gt_color[rayq * 3 + 1]; gtc[2] = P.gt_color[rayq * 3 + 2]; }
        double qx = 0.0, qy = 0.0, qz = 0.0, zq = 0.0;
        F4 rw = F4{0.f, 0.f, 0.f, 0.f};
        bool ins = true;
        if (act) {
            const double *pq = P.pd + gq * 4;
            qx = pq[0]; qy = pq[1]; qz = pq[2]; zq = pq[3];
            const float *scr = P.draw + gq * 4;
            float occ = scr[0];
            if (STAGE >= NSR_STAGE_FINE) occ = scr[1] + scr[0];                             // decoder.py:333,341
            if (STAGE == NSR_STAGE_COLOR) { const float *rc = P.raw + gq * 4; rw.x = rc[0]; rw.y = rc[1]; rw.z = rc[2]; }
            ins = in_bound(P, qx, qy, qz);
            rw.w = ins ? occ : 100.f;                                                       // Renderer.py:57
            st4(P.raw + gq * 4, rw);
        }
        const Comp c = comp_weights(rw.w, act, lane);
        const RayOut o = composite(c, rw, zq);
        if (lane == 0) {
            P.depth[rayq] = o.depth;
            P.var[rayq] = o.var;
            P.rgb[rayq * 3 + 0] = o.cr; P.rgb[rayq * 3 + 1] = o.cg; P.rgb[rayq * 3 + 2] = o.cb;
        }
        if (P.loss) {
            const RayLoss L = mapping_loss_ray<STAGE>(P, kp, gd, gtc, o.depth, o.cr, o.cg, o.cb);
            lterm = L.term;
            if (lane == 0) {
                if (P.dl_depth) P.dl_depth[rayq] = L.gD;
                if (P.dl_rgb) { P.dl_rgb[rayq * 3 + 0] = L.g3[0]; P.dl_rgb[rayq * 3 + 1] = L.g3[1]; P.dl_rgb[rayq * 3 + 2] = L.g3[2]; }
            }
            if (P.dl_depth) {
                // d raw per sample for the split backward: what comp_bwd_kernel writes for these gradients and d var = 0
                float docc = comp_docc(c, rw, zq, o.dz, L.gD, 0.0, L.g3[0], L.g3[1], L.g3[2], act, lane);
                if (!ins) docc = 0.f;
                if (act) st4(P.draw + gq * 4, F4{c.w * L.g3[0], c.w * L.g3[1], c.w * L.g3[2], docc});
            }
        }
    }
    if (P.loss) {                                                    // one atomic per block
        if (lane == 0) red[wave] = lterm;
        block_sync();
        if (tid() == 0) {
            double s = 0.0;
            for (int w = 0; w < nw; ++w) s += red[w];
            if (s != 0.0) atomic_add_global_d(P.loss, s);
        }
    }
}

}  // namespace nsr
