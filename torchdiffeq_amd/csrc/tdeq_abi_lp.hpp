// tdeq_abi_lp.hpp — host-side validation-free launchers of the bfloat16 / float16 kernels (tdeq_kernels_lp.hpp).
// Included by tdeq_abi.hip inside its anonymous namespace (uses stream_grid, aligned16 / all_aligned, check_launch, the
// flag / flags / terms helpers, NormSetup, CtrlBundle and finish_norm); the extern "C" entry points route dtype
// TDEQ_BF16 / TDEQ_F16 here after their own argument checks, with S = lp::BF16 or lp::F16.
//
// Host scalars follow the torch-op host path of the package (torchdiffeq_amd/_fallback.py, pinned bit for bit to the
// reference on the CPU): `rs<S>(x)` = a double rounded to float32 and then to the storage type (a 0-dim tensor of the
// state's type, or a Python number that ATen rounds first), `(float)x` = a second operand taken at float32 (opmath).
#pragma once

// (tdeq_kernels_lp.hpp is included by tdeq_abi.hip at file scope)

template <typename S>
inline float rs(double x) { return S::rnd((float)x); }

template <int NIN, int NOUT>
inline bool lp_aligned(const lp::MapArgs<NIN, NOUT>& a) {
    bool vec = true;
    for (int j = 0; j < NIN; ++j) vec = vec && aligned16(a.in[j]);
    for (int o = 0; o < NOUT; ++o) vec = vec && (o >= a.n_live || aligned16(a.out[o]));
    return vec;
}

// LEANABLE (the stage combines): the common launch shapes get map_kernel's LEAN instantiations — see there.
template <typename S, int NIN, int NOUT, typename F, bool LEANABLE = false>
int lp_launch_map(lp::MapArgs<NIN, NOUT>& a, const F& f, hipStream_t s, bool needs_prepare = true) {
    if (lp_aligned(a)) {
        const dim3 g(stream_grid(a.n / lp::kVec, kBlock)), b(kBlock);
        if constexpr (LEANABLE) {
            if ((int64_t)g.x * kBlock >= a.n / lp::kVec && a.n_fill == 0 && a.n_live == NOUT) {
                if (needs_prepare) hipLaunchKernelGGL((lp::map_kernel<S, NIN, NOUT, true, F, true, true>), g, b, 0, s, a, f);
                else hipLaunchKernelGGL((lp::map_kernel<S, NIN, NOUT, true, F, true, false>), g, b, 0, s, a, f);
                return check_launch();
            }
        }
        hipLaunchKernelGGL((lp::map_kernel<S, NIN, NOUT, true, F>), g, b, 0, s, a, f);
    } else {
        hipLaunchKernelGGL((lp::map_kernel<S, NIN, NOUT, false, F>), dim3(stream_grid(a.n, kBlock)), dim3(kBlock), 0, s, a, f);
    }
    return check_launch();
}

template <int NIN, int NOUT>
inline void lp_no_fill(lp::MapArgs<NIN, NOUT>& a, int64_t n) {
    a.n = n;
    a.n_live = NOUT;
    a.fill_dst = nullptr;
    a.n_fill = 0;
    for (int i = 0; i < 16; ++i) a.fill_v[i] = 0;
}

// The terms of a launch: in[j] = k[j] and c_j = fl_S(fl_S(coef_j) * fl_S(dt)) — rk_common.py:79,201-205 (a stage row),
// :89 (dt * c_error), :365-366 (dt * c_mid); with dt in device memory (`dev_dt`: captured steps) c_j = fl_S(coef_j) and
// the kernel multiplies by the device's dt.
template <typename S, int NT>
inline void lp_fill_terms(const uint16_t** in, float* c, const void* const* k, const double* coef, double dt,
                          bool dev_dt = false) {
    const float dtS = rs<S>(dt);
    for (int j = 0; j < NT; ++j) {
        in[j] = static_cast<const uint16_t*>(k[j]);
        c[j] = dev_dt ? rs<S>(coef[j]) : S::rnd(rs<S>(coef[j]) * dtS);
    }
}

// ---- stage combines: out = y0 + row_sum, optionally a second row without y0 (the partial error) and the side fill ----
template <typename S, int NT, int NOUT>
int lp_launch_combine(void* out, void* err_out, const void* y0, const void* const* k, const double* coef,
                      const double* err_coef, double dt, int64_t n, hipStream_t s, const double* ctrl_dev = nullptr,
                      void* fill_dst = nullptr, const double* fill_vals = nullptr, int n_fill = 0) {
    lp::MapArgs<NT + 1, NOUT> a;
    lp_no_fill(a, n);
    lp::CombineF<S, NT, NOUT> f;
    a.in[0] = static_cast<const uint16_t*>(y0);
    lp_fill_terms<S, NT>(a.in + 1, f.c[0], k, coef, dt, ctrl_dev != nullptr);
    if (NOUT == 2) lp_fill_terms<S, NT>(a.in + 1, f.c[NOUT - 1], k, err_coef, dt, ctrl_dev != nullptr);
    a.out[0] = static_cast<uint16_t*>(out);
    if (NOUT == 2) a.out[NOUT - 1] = static_cast<uint16_t*>(err_out);
    f.ctrl_dev = ctrl_dev;
    if (fill_dst) {
        a.fill_dst = static_cast<uint16_t*>(fill_dst);
        a.n_fill = n_fill;
        for (int i = 0; i < n_fill; ++i) a.fill_v[i] = (uint16_t)S::st((float)fill_vals[i]);
    }
    return lp_launch_map<S, NT + 1, NOUT, lp::CombineF<S, NT, NOUT>, true>(a, f, s, ctrl_dev != nullptr);
}

// ---- error norm: the sum of fl_S(|r|^2) per segment (|r| itself for a one-element segment) + the non-finite census ----
template <typename S, int NT>
int lp_launch_error(void* scaled, const void* y0, const void* y1, const void* const* k, const double* coef, double dt,
                    const NormSetup& ns, double* out_sumsq, double* out_bad, const CtrlBundle* cb = nullptr) {
    lp::ErrArgs<NT> a;
    a.scaled = static_cast<uint16_t*>(scaled);
    a.y0 = static_cast<const uint16_t*>(y0);
    a.y1 = static_cast<const uint16_t*>(y1);
    const bool dev_dt = cb && cb->state_in_dev;
    lp_fill_terms<S, NT>(a.k, a.c, k, coef, dt, dev_dt);
    const bool vec = all_aligned(y0, y1, scaled, Ptrs{k, NT}) && (ns.st.chunk % lp::kVec == 0);
    a.ctrl_dev = dev_dt ? cb->ctrl_dev : nullptr;
    a.st = ns.st;
    a.part_sumsq = ns.ws;
    a.part_bad = ns.ws + 2 * ns.st.n_chunks;
    const dim3 g((unsigned)ns.st.n_chunks), b(kBlock);
    const bool single = ns.st.n_seg == 1 && ns.st.inl[0].chunk_start == 0;
    if (scaled || !vec || !single)
        flags(vec, scaled != nullptr, [&](auto v, auto sc) {
            hipLaunchKernelGGL((lp::error_norm_kernel<S, NT, decltype(v)::value, decltype(sc)::value>), g, b, 0, ns.s, a);
            return 0;
        });
    else if (!dev_dt) hipLaunchKernelGGL((lp::error_norm_kernel<S, NT, true, false, true, false>), g, b, 0, ns.s, a);
    else hipLaunchKernelGGL((lp::error_norm_kernel<S, NT, true, false, true, true>), g, b, 0, ns.s, a);
    // with a controller bundle: finalize + the step controller in the state's type (tkind 2 / 3), as for fp32 / fp64
    return finish_norm(ns, 1, out_sumsq, out_bad, cb, kTkind<S>);
}

// ---- initial-step quotients: their sums (out0 == nullptr) or the quotients themselves (no workspace) ----
template <typename S>
int lp_launch_init(int mode, const void* a_, const void* b_, const void* y, const NormSetup& ns, double* out_sumsq,
                   double* out_bad, void* out0, void* out1) {
    lp::InitArgs a;
    a.a = static_cast<const uint16_t*>(a_);
    a.b = static_cast<const uint16_t*>(b_);
    a.y = static_cast<const uint16_t*>(y);
    a.st = ns.st;
    a.part0 = ns.ws;
    a.part1 = ns.ws ? ns.ws + ns.st.n_chunks : nullptr;
    a.part_bad = ns.ws ? ns.ws + 2 * ns.st.n_chunks : nullptr;
    a.out0 = static_cast<uint16_t*>(out0);
    a.out1 = static_cast<uint16_t*>(out1);
    const dim3 g((unsigned)ns.st.n_chunks), b(kBlock);
    flags(mode != 0, out0 != nullptr, [&](auto m, auto o) {
        hipLaunchKernelGGL((lp::init_norms_kernel<S, decltype(m)::value ? 1 : 0, decltype(o)::value>), g, b, 0, ns.s, a);
        return 0;
    });
    if (out0) return check_launch();
    return finish_norm(ns, mode == 0 ? 2 : 1, out_sumsq, out_bad);
}

// ---- dense output ----
// the inputs of the quartic's fit: y0, y1, f0, f1, the k_j with c_j = dt * c_mid_j, and dt, 2 dt as the fit rounds them
template <typename S, int NT, int NOUT, typename F>
inline void lp_fill_dense(lp::MapArgs<NT + 4, NOUT>& a, F& f, const void* y0, const void* y1, const void* f0, const void* f1,
                          const void* const* k, const double* coef, double dt, int64_t n) {
    lp_no_fill(a, n);
    a.in[0] = static_cast<const uint16_t*>(y0);
    a.in[1] = static_cast<const uint16_t*>(y1);
    a.in[2] = static_cast<const uint16_t*>(f0);
    a.in[3] = static_cast<const uint16_t*>(f1);
    lp_fill_terms<S, NT>(a.in + 4, f.cm, k, coef, dt);
    f.dt = rs<S>(dt);
    f.two_dt = S::rnd(2.0f * f.dt);
}

template <typename S, int NT, int M>
int lp_launch_dense_eval(void* out, int64_t out_stride, const void* y0, const void* y1, const void* f0, const void* f1,
                         const void* const* k, const double* coef, double dt, const double* x, int n_x, int64_t n,
                         hipStream_t s) {
    lp::MapArgs<NT + 4, M> a;
    lp::DenseEvalF<S, NT, M> f;
    lp_fill_dense<S, NT>(a, f, y0, y1, f0, f1, k, coef, dt, n);
    a.n_live = n_x;
    for (int m = 0; m < M; ++m) {
        a.out[m] = static_cast<uint16_t*>(out) + (int64_t)(m < n_x ? m : 0) * out_stride;
        const float xS = rs<S>(m < n_x ? x[m] : 0.0);       // interp.py:40: x cast to the state's type
        f.xp[m][0] = xS;
        f.xp[m][1] = S::rnd(xS * xS);                        // interp.py:42-47: x_power *= x
        f.xp[m][2] = S::rnd(f.xp[m][1] * xS);
        f.xp[m][3] = S::rnd(f.xp[m][2] * xS);
    }
    return lp_launch_map<S, NT + 4, M>(a, f, s);
}

template <typename S>
int lp_dense_eval(void* out, int64_t out_stride, const void* y0, const void* y1, const void* f0, const void* f1,
                  const void* const* k, const double* coef, int nt, double dt, const double* x, int n_x, int64_t n,
                  hipStream_t s) {
    // one row, or groups of up to 4 (the quartic is re-fitted per group — output rows stay bit-identical)
    auto rows = [&](auto m, int lo, int n_rows) {
        return terms<1>(nt, [&](auto t) {
            return lp_launch_dense_eval<S, decltype(t)::value, decltype(m)::value>(
                static_cast<uint16_t*>(out) + (int64_t)lo * out_stride, out_stride, y0, y1, f0, f1, k, coef, dt, x + lo, n_rows, n, s);
        });
    };
    if (n_x == 1) return rows(std::integral_constant<int, 1>{}, 0, 1);
    for (int lo = 0; lo < n_x; lo += 4) {
        const int e = rows(std::integral_constant<int, 4>{}, lo, n_x - lo < 4 ? n_x - lo : 4);
        if (e) return e;
    }
    return 0;
}

template <typename S, int NT>
int lp_launch_fit(void* coeffs, const void* y0, const void* y1, const void* f0, const void* f1, const void* const* k,
                  const double* coef, double dt, int64_t n, hipStream_t s) {
    lp::MapArgs<NT + 4, 5> a;
    lp::DenseFitF<S, NT> f;
    lp_fill_dense<S, NT>(a, f, y0, y1, f0, f1, k, coef, dt, n);
    for (int p = 0; p < 5; ++p) a.out[p] = static_cast<uint16_t*>(coeffs) + (int64_t)p * n;
    return lp_launch_map<S, NT + 4, 5>(a, f, s);
}

// ---- fixed-grid stages ----
// (a stage reads k1..k<STAGE>: the entry point has checked those)
template <typename S, int STAGE>
int lp_launch_rk4(void* out, const void* y0, const void* const (&ks)[4], double dt, int64_t n, hipStream_t s) {
    lp::MapArgs<STAGE + 1, 1> a;
    lp_no_fill(a, n);
    a.in[0] = static_cast<const uint16_t*>(y0);
    for (int j = 0; j < STAGE; ++j) a.in[1 + j] = static_cast<const uint16_t*>(ks[j]);
    a.out[0] = static_cast<uint16_t*>(out);
    lp::Rk4F<S, STAGE> f;
    f.dt_first = rs<S>(dt);
    f.dt_second = (float)dt;
    f.third = (float)(1.0 / 3.0);
    return lp_launch_map<S, STAGE + 1, 1>(a, f, s);
}

template <typename S>
int lp_launch_lerp(void* out, const void* y0, const void* y1, double slope, int64_t n, hipStream_t s) {
    lp::MapArgs<2, 1> a;
    lp_no_fill(a, n);
    a.in[0] = static_cast<const uint16_t*>(y0);
    a.in[1] = static_cast<const uint16_t*>(y1);
    a.out[0] = static_cast<uint16_t*>(out);
    lp::LerpF<S> f;
    f.slope = rs<S>(slope);
    return lp_launch_map<S, 2, 1>(a, f, s);
}

template <typename S, int NT, int MODE>
int lp_launch_fixed(void* out, const void* y0, const void* const* k, const double* w, double dt, int64_t n, hipStream_t s) {
    lp::MapArgs<NT + 1, 1> a;
    lp_no_fill(a, n);
    a.in[0] = static_cast<const uint16_t*>(y0);
    lp::FixedF<S, NT, MODE> f;
    for (int j = 0; j < NT; ++j) {
        a.in[1 + j] = static_cast<const uint16_t*>(k[j]);
        f.w[j] = (float)w[j];
    }
    f.dt = rs<S>(dt);
    a.out[0] = static_cast<uint16_t*>(out);
    return lp_launch_map<S, NT + 1, 1>(a, f, s);
}

template <typename S, int NT>
int lp_launch_weighted(void* out, const void* const* x, const double* w, int64_t n, hipStream_t s) {
    lp::MapArgs<NT, 1> a;
    lp_no_fill(a, n);
    lp::WeightedF<S, NT> f;
    for (int j = 0; j < NT; ++j) {
        a.in[j] = static_cast<const uint16_t*>(x[j]);
        f.w[j] = rs<S>(w[j]);
    }
    a.out[0] = static_cast<uint16_t*>(out);
    return lp_launch_map<S, NT, 1>(a, f, s);
}

// ---- look-ahead first stage ----
template <typename S>
int lp_launch_sel(void* out, const void* y_acc, const void* f_acc, const void* y_rej, const void* f_rej, double coef,
                  const double* ctrl_dev, int64_t n, hipStream_t s) {
    lp::SelArgs a;
    a.out = static_cast<uint16_t*>(out);
    a.y_acc = static_cast<const uint16_t*>(y_acc);
    a.f_acc = static_cast<const uint16_t*>(f_acc);
    a.y_rej = static_cast<const uint16_t*>(y_rej);
    a.f_rej = static_cast<const uint16_t*>(f_rej);
    a.coef = rs<S>(coef);
    a.ctrl_dev = ctrl_dev;
    a.n = n;
    const bool vec = all_aligned(out, y_acc, f_acc, y_rej, f_rej);
    const dim3 g(stream_grid(vec ? n / lp::kVec : n, kBlock));
    return flag(vec, [&](auto v) {
        hipLaunchKernelGGL((lp::sel_kernel<S, decltype(v)::value>), g, dim3(kBlock), 0, s, a);
        return check_launch();
    });
}
