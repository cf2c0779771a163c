// C handle layer (include/cuddh_capi.h).  Compiled as HIP: the built-in integrands
// are device functors fed to the LinearFunctional header templates.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <exception>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "cuddh.hpp"
#include "cuddh_capi.h"
#include "cuddh_hip.h"
#include "gmres_small.hpp"

using namespace cuddh;

namespace
{
    thread_local std::string g_error;

    template <typename F>
    int guarded(F &&f)
    {
        try
        {
            f();
            return 0;
        }
        catch (const std::exception &e)
        {
            g_error = e.what();
        }
        catch (...)
        {
            g_error = "unknown error";
        }
        return 1;
    }

    // checked before anything touches the device
    Orthogonalization orth_of(int orth)
    {
        if (orth == 0)
            return Orthogonalization::mgs;
        if (orth == 1)
            return Orthogonalization::cgs2;
        throw std::runtime_error("gmres error: orthogonalization must be 0 (mgs) or 1 (cgs2), not " + std::to_string(orth) + ".");
    }

    // likewise: orth as above, augment in [0, m - 1]
    GmresOptions options_of(int orth, int augment, int m)
    {
        GmresOptions o;
        o.orth = orth_of(orth);
        if (augment < 0 || (augment > 0 && augment >= m))
            throw std::runtime_error("gmres error: augment must be in [0, m - 1], not " + std::to_string(augment) + ".");
        o.augment = augment;
        return o;
    }

    template <typename T, typename F>
    T *guarded_new(F &&f)
    {
        T *out = nullptr;
        guarded([&] { out = f(); });
        return out;
    }

    struct Integrand
    {
        int id;
        double param;

        __host__ __device__ double operator()(const double X[2]) const
        {
            const double x = X[0], y = X[1];
            switch (id)
            {
            case 0:
            {
                const double s = param * param;
                double r = (x + 0.5) * (x + 0.5) + y * y;
                double F = s / M_PI * exp(-s * r);
                r = (x - 0.5) * (x - 0.5) + (y + 0.5) * (y + 0.5);
                return F + s / M_PI * exp(-s * r);
            }
            case 1: return (x * x + y * y < 0.0625) ? 0.2 : 1.0;
            case 2: return 3.0 * x * x - 2.0 * x * y + y + 1.0;
            case 3:
            {
                const double x3 = x * x * x, x5 = x3 * x * x, y3 = y * y * y;
                return -6.0 * y * (x5 - 5.0 * x) - 20.0 * x3 * (y3 - 3.0 * y);
            }
            case 4:
            {
                const double x5 = x * x * x * x * x, y3 = y * y * y;
                return (x5 - 5.0 * x) * (y3 - 3.0 * y);
            }
            case 5: return param;
            case 6:
            {
                const double a = (x * x + y * y < 0.0625) ? 0.2 : 1.0;
                return a * a;
            }
            default: return 0.0;
            }
        }
    };

    struct OpHandle
    {
        std::unique_ptr<Operator> op;
        HelmholtzOperator *helm = nullptr; // non-owning view when op is a HelmholtzOperator
    };

    struct DdhHandle
    {
        std::unique_ptr<DDH> f32;
        std::unique_ptr<DDH64> f64;
        bool is64() const { return static_cast<bool>(f64); }
    };

    void fill_result(const solver_out &o, cuddh_solver_result *out, double *h_res, double *h_time)
    {
        if (out)
        {
            out->success = o.success ? 1 : 0;
            out->num_iter = o.num_iter;
            out->num_matvec = o.num_matvec;
            out->n_res = static_cast<int>(o.res_norm.size());
        }
        for (std::size_t i = 0; i < o.res_norm.size(); ++i)
        {
            if (h_res)
                h_res[i] = o.res_norm[i];
            if (h_time)
                h_time[i] = o.time[i];
        }
    }

    class CallbackOp64 : public Operator
    {
    public:
        CallbackOp64(cuddh_action_cb cb_, void *ctx_) : cb(cb_), ctx(ctx_) {}
        void action(const double *x, double *y) const override { cb(ctx, x, y); }
        void action(double, const double *, double *) const override { cuddh_error("callback operator: action(c,x,y) unsupported"); }

    private:
        cuddh_action_cb cb;
        void *ctx;
    };

    class CallbackOp32 : public SinglePrecisionOperator
    {
    public:
        CallbackOp32(cuddh_action_cb cb_, void *ctx_) : cb(cb_), ctx(ctx_) {}
        void action(const float *x, float *y) const override { cb(ctx, x, y); }

    private:
        cuddh_action_cb cb;
        void *ctx;
    };

    template <typename T>
    long long copy_table(const HostDeviceArray<T> &t, void *h_out, int count_only)
    {
        if (!count_only && t.size() > 0)
            std::memcpy(h_out, t.host_read(), sizeof(T) * static_cast<std::size_t>(t.size()));
        return t.size();
    }

    template <typename Real>
    long long ddh_table(const detail::DDHCore<Real> &c, const std::string &name, void *h_out, int count_only)
    {
        if (name == "B") return copy_table(c.table_B(), h_out, count_only);
        if (name == "gI") return copy_table(c.table_gI(), h_out, count_only);
        if (name == "sI") return copy_table(c.table_sI(), h_out, count_only);
        if (name == "D") return copy_table(c.table_D(), h_out, count_only);
        if (name == "G") return copy_table(c.table_G(), h_out, count_only);
        if (name == "m") return copy_table(c.table_m(), h_out, count_only);
        if (name == "gmi") return copy_table(c.table_gmi(), h_out, count_only);
        if (name == "a") return copy_table(c.table_a(), h_out, count_only);
        if (name == "H") return copy_table(c.table_H(), h_out, count_only);
        if (name == "filter") return copy_table(c.table_filter(), h_out, count_only);
        if (name == "cs") return copy_table(c.table_cs(), h_out, count_only);
        if (name == "sn") return copy_table(c.table_sn(), h_out, count_only);
        // "filter@R", "cs@R", "sn@R": the tables of the time grid of R times the mesh grid's steps
        if (const std::size_t at = name.find('@'); at != std::string::npos)
        {
            const std::string base = name.substr(0, at), ratio = name.substr(at + 1);
            const int which = base == "filter" ? 0 : base == "cs" ? 1 : base == "sn" ? 2 : -1;
            if (which >= 0 && !ratio.empty() && ratio.size() <= 4 && ratio.find_first_not_of("0123456789") == std::string::npos)
            {
                const Real *table = nullptr;
                const long long n = c.time_grid_table(std::stoi(ratio), which, table);
                if (n == 0)
                    throw std::runtime_error("DDH table " + name + ": no subdomain marches on that time grid");
                if (!count_only)
                    std::memcpy(h_out, table, sizeof(Real) * static_cast<std::size_t>(n));
                return n;
            }
        }
        throw std::runtime_error("unknown DDH table: " + name);
    }
} // namespace

extern "C"
{
    const char *cuddh_last_error(void) { return g_error.c_str(); }

    void cuddh_set_stream(void *s) { set_stream(static_cast<hipStream_t>(s)); }
    void *cuddh_get_stream(void) { return stream(); }

    // ------------------------------------------------------------ quadrature / basis
    int cuddh_quadrature(int n, int type, double *h_x, double *h_w)
    {
        return guarded([&]
        {
            QuadratureRule q(n, type == 0 ? QuadratureRule::GaussLegendre : QuadratureRule::GaussLobatto);
            for (int i = 0; i < n; ++i)
            {
                h_x[i] = q.x(i);
                h_w[i] = q.w(i);
            }
        });
    }

    void *cuddh_basis_create(int n) { return guarded_new<Basis>([&] { return new Basis(n); }); }
    void cuddh_basis_destroy(void *b) { delete static_cast<Basis *>(b); }
    int cuddh_basis_eval(void *b, int m, const double *h_x, double *h_P)
    {
        return guarded([&] { static_cast<Basis *>(b)->eval(m, h_x, h_P); });
    }
    int cuddh_basis_deriv(void *b, int m, const double *h_x, double *h_D)
    {
        return guarded([&] { static_cast<Basis *>(b)->deriv(m, h_x, h_D); });
    }

    // ------------------------------------------------------------ mesh
    void *cuddh_mesh_uniform_rect(int nx, double ax, double bx, int ny, double ay, double by)
    {
        return guarded_new<Mesh2D>([&] { return new Mesh2D(Mesh2D::uniform_rect(nx, ax, bx, ny, ay, by)); });
    }
    void *cuddh_mesh_grid_cells(int nx, double ax, double bx, int ny, double ay, double by, const unsigned char *h_present)
    {
        return guarded_new<Mesh2D>([&] { return new Mesh2D(grid_cells(nx, ax, bx, ny, ay, by, h_present)); });
    }
    void *cuddh_mesh_from_vertices(int n_pts, const double *h_xy, int n_elem, const int *h_elems)
    {
        return guarded_new<Mesh2D>([&] { return new Mesh2D(Mesh2D::from_vertices(n_pts, h_xy, n_elem, h_elems)); });
    }
    void *cuddh_mesh_load(const char *dir)
    {
        return guarded_new<Mesh2D>([&] { return new Mesh2D(load_mesh(dir)); });
    }
    void *cuddh_mesh_refined(void *m, int times)
    {
        return guarded_new<Mesh2D>([&]
        {
            const QuadMeshData fine = refine_quads(mesh_data(*static_cast<Mesh2D *>(m)), times);
            return new Mesh2D(Mesh2D::from_vertices(fine.n_pts(), fine.xy.data(), fine.n_elem(), fine.elems.data()));
        });
    }
    int cuddh_mesh_partition(void *m, int n_parts, int *h_labels)
    {
        return guarded([&]
        {
            const std::vector<int> labels = partition_elements(*static_cast<Mesh2D *>(m), n_parts);
            std::copy(labels.begin(), labels.end(), h_labels);
        });
    }
    void cuddh_mesh_destroy(void *m) { delete static_cast<Mesh2D *>(m); }
    int cuddh_mesh_n_elem(void *m) { return static_cast<Mesh2D *>(m)->n_elem(); }
    int cuddh_mesh_n_edges(void *m) { return static_cast<Mesh2D *>(m)->n_edges(); }
    int cuddh_mesh_n_nodes(void *m) { return static_cast<Mesh2D *>(m)->n_nodes(); }
    int cuddh_mesh_n_boundary_edges(void *m) { return static_cast<Mesh2D *>(m)->n_edges(FaceType::BOUNDARY); }
    int cuddh_mesh_boundary_edges(void *m, int *h_out)
    {
        return guarded([&]
        {
            ivec b = static_cast<Mesh2D *>(m)->boundary_edges();
            for (int i = 0; i < b.size(); ++i)
                h_out[i] = b[i];
        });
    }
    int cuddh_mesh_edges(void *m, int *h_out)
    {
        return guarded([&]
        {
            const Mesh2D *mesh = static_cast<Mesh2D *>(m);
            for (int e = 0; e < mesh->n_edges(); ++e)
            {
                const Edge *ed = mesh->edge(e);
                int *o = h_out + 8 * e;
                o[0] = ed->type == FaceType::BOUNDARY ? 1 : 0;
                o[1] = ed->nodes[0];
                o[2] = ed->nodes[1];
                o[3] = ed->elements[0];
                o[4] = ed->elements[1];
                o[5] = ed->sides[0];
                o[6] = ed->sides[1];
                o[7] = ed->delta;
            }
        });
    }
    double cuddh_mesh_min_h(void *m) { return static_cast<Mesh2D *>(m)->min_h(); }
    int cuddh_mesh_vertices(void *m, double *h_xy)
    {
        return guarded([&]
        {
            const Mesh2D *mesh = static_cast<Mesh2D *>(m);
            for (int i = 0; i < mesh->n_nodes(); ++i)
            {
                h_xy[2 * i] = mesh->node(i).x[0];
                h_xy[2 * i + 1] = mesh->node(i).x[1];
            }
        });
    }
    int cuddh_mesh_elements(void *m, int *h_out)
    {
        return guarded([&]
        {
            const Mesh2D *mesh = static_cast<Mesh2D *>(m);
            for (int e = 0; e < mesh->n_elem(); ++e)
                for (int c = 0; c < 4; ++c)
                    h_out[4 * e + c] = mesh->element(e)->nodes[c];
        });
    }

    // ------------------------------------------------------------ spaces
    void *cuddh_h1space_create(void *mesh, void *basis)
    {
        return guarded_new<H1Space>([&] { return new H1Space(*static_cast<Mesh2D *>(mesh), *static_cast<Basis *>(basis)); });
    }
    void cuddh_h1space_destroy(void *f) { delete static_cast<H1Space *>(f); }
    int cuddh_h1space_size(void *f) { return static_cast<H1Space *>(f)->size(); }
    int cuddh_h1space_global_indices(void *f, int *h_I)
    {
        return guarded([&]
        {
            auto I = static_cast<H1Space *>(f)->global_indices(MemorySpace::HOST);
            std::memcpy(h_I, I.data(), sizeof(int) * static_cast<std::size_t>(I.size()));
        });
    }
    int cuddh_h1space_coordinates(void *f, double *h_xy)
    {
        return guarded([&]
        {
            auto X = static_cast<H1Space *>(f)->physical_coordinates(MemorySpace::HOST);
            std::memcpy(h_xy, X.data(), sizeof(double) * static_cast<std::size_t>(X.size()));
        });
    }
    const int *cuddh_h1space_global_indices_device(void *f)
    {
        const int *p = nullptr;
        guarded([&] { p = static_cast<H1Space *>(f)->global_indices(MemorySpace::DEVICE).data(); });
        return p;
    }
    const double *cuddh_h1space_coordinates_device(void *f)
    {
        const double *p = nullptr;
        guarded([&] { p = static_cast<H1Space *>(f)->physical_coordinates(MemorySpace::DEVICE).data(); });
        return p;
    }

    void *cuddh_facespace_create(void *fem, int n_faces, const int *h_faces)
    {
        return guarded_new<FaceSpace>([&] { return new FaceSpace(*static_cast<H1Space *>(fem), n_faces, h_faces); });
    }
    void cuddh_facespace_destroy(void *fs) { delete static_cast<FaceSpace *>(fs); }
    int cuddh_facespace_size(void *fs) { return static_cast<FaceSpace *>(fs)->size(); }
    int cuddh_facespace_subspace_indices(void *fs, int *h_I)
    {
        return guarded([&]
        {
            auto I = static_cast<FaceSpace *>(fs)->subspace_indices(MemorySpace::HOST);
            std::memcpy(h_I, I.data(), sizeof(int) * static_cast<std::size_t>(I.size()));
        });
    }
    int cuddh_facespace_global_indices(void *fs, int *h_proj)
    {
        return guarded([&]
        {
            auto I = static_cast<FaceSpace *>(fs)->global_indices(MemorySpace::HOST);
            std::memcpy(h_proj, I.data(), sizeof(int) * static_cast<std::size_t>(I.size()));
        });
    }
    int cuddh_facespace_restrict(void *fs, const double *x, double *y) { return guarded([&] { static_cast<FaceSpace *>(fs)->restrict(x, y); }); }
    int cuddh_facespace_prolong(void *fs, const double *x, double *y) { return guarded([&] { static_cast<FaceSpace *>(fs)->prolong(x, y); }); }
    int cuddh_facespace_orth(void *fs, double *x) { return guarded([&] { static_cast<FaceSpace *>(fs)->orth(x); }); }

    // ------------------------------------------------------------ EnsembleSpace
    void *cuddh_ensemble_create(void *fem, int n_spaces, const int *h_labels)
    {
        return guarded_new<EnsembleSpace>([&] { return new EnsembleSpace(*static_cast<H1Space *>(fem), n_spaces, h_labels); });
    }
    void cuddh_ensemble_destroy(void *e) { delete static_cast<EnsembleSpace *>(e); }
    int cuddh_ensemble_dims(void *e, int *d)
    {
        return guarded([&]
        {
            const EnsembleSpace *E = static_cast<EnsembleSpace *>(e);
            d[0] = E->size();
            d[1] = E->elements(MemorySpace::HOST).shape(0);
            d[2] = E->faces(MemorySpace::HOST).shape(0);
            d[3] = E->global_indices(MemorySpace::HOST).shape(0);
            d[4] = E->face_proj(MemorySpace::HOST).shape(0);
            d[5] = E->connectivity_map(MemorySpace::HOST).shape(1);
        });
    }
    int cuddh_ensemble_array(void *e, const char *name_, int *h_out)
    {
        return guarded([&]
        {
            const EnsembleSpace *E = static_cast<EnsembleSpace *>(e);
            const std::string name(name_);
            const int *src = nullptr;
            int n = 0;
            auto take = [&](auto w)
            {
                src = w.data();
                n = w.size();
            };
            if (name == "gI") take(E->global_indices(MemorySpace::HOST));
            else if (name == "sizes") take(E->sizes(MemorySpace::HOST));
            else if (name == "elements") take(E->elements(MemorySpace::HOST));
            else if (name == "n_elems") take(E->n_elems(MemorySpace::HOST));
            else if (name == "faces") take(E->faces(MemorySpace::HOST));
            else if (name == "n_faces") take(E->n_faces(MemorySpace::HOST));
            else if (name == "sI") take(E->subspace_indices(MemorySpace::HOST));
            else if (name == "fI") take(E->face_indices(MemorySpace::HOST));
            else if (name == "pI") take(E->face_proj(MemorySpace::HOST));
            else if (name == "fsizes") take(E->fsizes(MemorySpace::HOST));
            else if (name == "cmap") take(E->connectivity_map(MemorySpace::HOST));
            else throw std::runtime_error("unknown EnsembleSpace array: " + name);
            if (n > 0)
                std::memcpy(h_out, src, sizeof(int) * static_cast<std::size_t>(n));
        });
    }

    // ------------------------------------------------------------ operators
    void *cuddh_stiffness_create(void *fem, int nq)
    {
        return guarded_new<OpHandle>([&]
        {
            auto h = new OpHandle;
            const H1Space &f = *static_cast<H1Space *>(fem);
            if (nq > 0)
                h->op.reset(new StiffnessMatrix(f, QuadratureRule(nq, QuadratureRule::GaussLegendre)));
            else
                h->op.reset(new StiffnessMatrix(f));
            return h;
        });
    }
    void *cuddh_mass_create(void *fem, const double *coef)
    {
        return guarded_new<OpHandle>([&]
        {
            auto h = new OpHandle;
            const H1Space &f = *static_cast<H1Space *>(fem);
            h->op.reset(coef ? new MassMatrix(coef, f) : new MassMatrix(f));
            return h;
        });
    }
    void *cuddh_diaginv_mass_create(void *fem, const double *coef)
    {
        return guarded_new<OpHandle>([&]
        {
            auto h = new OpHandle;
            const H1Space &f = *static_cast<H1Space *>(fem);
            h->op.reset(coef ? new DiagInvMassMatrix(coef, f) : new DiagInvMassMatrix(f));
            return h;
        });
    }
    void *cuddh_facemass_create(void *fs, const double *coef)
    {
        return guarded_new<OpHandle>([&]
        {
            auto h = new OpHandle;
            const FaceSpace &f = *static_cast<FaceSpace *>(fs);
            h->op.reset(coef ? new FaceMassMatrix(coef, f) : new FaceMassMatrix(f));
            return h;
        });
    }
    void *cuddh_diaginv_facemass_create(void *fs, const double *coef)
    {
        return guarded_new<OpHandle>([&]
        {
            auto h = new OpHandle;
            const FaceSpace &f = *static_cast<FaceSpace *>(fs);
            h->op.reset(coef ? new DiagInvFaceMassMatrix(coef, f) : new DiagInvFaceMassMatrix(f));
            return h;
        });
    }
    void *cuddh_helmholtz_create(double omega, const double *a2x, const double *ax, void *fem, void *fs)
    {
        return guarded_new<OpHandle>([&]
        {
            auto h = new OpHandle;
            auto *H = new HelmholtzOperator(omega, a2x, ax, *static_cast<H1Space *>(fem), *static_cast<FaceSpace *>(fs));
            h->op.reset(H);
            h->helm = H;
            return h;
        });
    }
    void cuddh_operator_destroy(void *op) { delete static_cast<OpHandle *>(op); }
    int cuddh_operator_apply(void *op, const double *x, double *y) { return guarded([&] { static_cast<OpHandle *>(op)->op->action(x, y); }); }
    int cuddh_operator_apply_add(void *op, double c, const double *x, double *y)
    {
        return guarded([&] { static_cast<OpHandle *>(op)->op->action(c, x, y); });
    }
    int cuddh_helmholtz_apply_unfused(void *op, const double *x, double *y)
    {
        return guarded([&]
        {
            auto *h = static_cast<OpHandle *>(op);
            if (!h->helm)
                throw std::runtime_error("not a Helmholtz operator");
            h->helm->action_unfused(x, y);
        });
    }
    int cuddh_helmholtz_is_fused(void *op)
    {
        auto *h = static_cast<OpHandle *>(op);
        return h->helm && h->helm->fused() ? 1 : 0;
    }
    int cuddh_operator_kernel_name(void *op, char *buf, int cap)
    {
        return guarded([&]
        {
            auto *h = static_cast<OpHandle *>(op);
            std::string name = "generic";
            if (h->helm)
                name = h->helm->kernel_name();
            else if (auto *s = dynamic_cast<StiffnessMatrix *>(h->op.get()))
                name = s->kernel_name();
            else if (auto *m = dynamic_cast<MassMatrix *>(h->op.get()))
                name = m->kernel_name();
            else if (auto *wh = dynamic_cast<WaveHoltz *>(h->op.get()))
                name = wh->stiffness_kernel();
            else if (auto *wb = dynamic_cast<WaveHoltzBox *>(h->op.get()))
                name = wb->stiffness_kernel();
            std::snprintf(buf, cap, "%s", name.c_str());
        });
    }
    // ------------------------------------------------------------ whole-domain WaveHoltz
    void *cuddh_waveholtz_create(double omega, const double *h_a, void *fem, int integrator, int coarsen, int time_ratio, int stiffness,
                                 const int *h_faces, int n_faces)
    {
        return cuddh_waveholtz_create_sweep(omega, h_a, fem, integrator, coarsen, time_ratio, stiffness, h_faces, n_faces, 0);
    }
    void *cuddh_waveholtz_create_sweep(double omega, const double *h_a, void *fem, int integrator, int coarsen, int time_ratio, int stiffness,
                                       const int *h_faces, int n_faces, int sweep)
    {
        return cuddh_waveholtz_create_precision(omega, h_a, fem, integrator, coarsen, time_ratio, stiffness, h_faces, n_faces, sweep, 0);
    }
    void *cuddh_waveholtz_create_precision(double omega, const double *h_a, void *fem, int integrator, int coarsen, int time_ratio, int stiffness,
                                           const int *h_faces, int n_faces, int sweep, int precision)
    {
        return cuddh_waveholtz_create_launch(omega, h_a, fem, integrator, coarsen, time_ratio, stiffness, h_faces, n_faces, sweep, precision, 0);
    }
    namespace
    {
        // cuddh_waveholtz_create_launch, and with h_beta cuddh_waveholtz_create_cell_stiffness
        void *waveholtz_create(double omega, const double *h_a, void *fem, int integrator, int coarsen, int time_ratio, int stiffness,
                               const int *h_faces, int n_faces, int sweep, int precision, int launch, const double *h_beta);
    } // namespace
    void *cuddh_waveholtz_create_launch(double omega, const double *h_a, void *fem, int integrator, int coarsen, int time_ratio, int stiffness,
                                        const int *h_faces, int n_faces, int sweep, int precision, int launch)
    {
        return waveholtz_create(omega, h_a, fem, integrator, coarsen, time_ratio, stiffness, h_faces, n_faces, sweep, precision, launch, nullptr);
    }
    void *cuddh_waveholtz_create_cell_stiffness(double omega, const double *h_a, void *fem, int integrator, int coarsen, int time_ratio, int stiffness,
                                                const int *h_faces, int n_faces, int sweep, int precision, int launch, const double *h_beta)
    {
        if (!h_beta)
            return guarded_new<OpHandle>([&]() -> OpHandle *
                                         { throw std::runtime_error("WaveHoltz error: cell_stiffness: no values were given (NULL)."); });
        return waveholtz_create(omega, h_a, fem, integrator, coarsen, time_ratio, stiffness, h_faces, n_faces, sweep, precision, launch, h_beta);
    }
    namespace
    {
    void *waveholtz_create(double omega, const double *h_a, void *fem, int integrator, int coarsen, int time_ratio, int stiffness,
                           const int *h_faces, int n_faces, int sweep, int precision, int launch, const double *h_beta)
    {
        return guarded_new<OpHandle>([&]
        {
            if (launch != 0 && launch != 1)
                throw std::runtime_error("WaveHoltz error: launch: the launch must be 0 (one per sweep) or 1 (one per pair of sweeps), not " +
                                         std::to_string(launch) + ".");
            if (launch == 1 && sweep != 1)
                throw std::runtime_error("WaveHoltz error: launch: pairs of sweeps are an option of the lattice form; they need sweep = 1 (lattice).");
            if (precision != 0 && precision != 1)
                throw std::runtime_error("WaveHoltz error: precision: the precision must be 0 (f64) or 1 (f32), not " + std::to_string(precision) + ".");
            if (precision == 1 && sweep == 0)
                throw std::runtime_error("WaveHoltz error: precision: f32 is an option of the lattice form; it needs sweep = 1 (lattice).");
            if (sweep != 0 && sweep != 1)
                throw std::runtime_error("WaveHoltz error: sweep: the form must be 0 (operator kernels) or 1 (lattice), not " + std::to_string(sweep) + ".");
            if (integrator != 0 && integrator != 1)
                throw std::runtime_error("WaveHoltz error: integrator: the scheme must be 0 (rk2) or 1 (rk4), not " + std::to_string(integrator) + ".");
            if (stiffness != 0 && stiffness != 1)
                throw std::runtime_error("WaveHoltz error: stiffness: the rule must be 0 (gauss) or 1 (lobatto), not " + std::to_string(stiffness) + ".");
            WaveHoltzOptions o;
            o.integrator = {integrator == 1 ? DDHIntegrator::rk4 : DDHIntegrator::rk2, coarsen};
            o.time_ratio = time_ratio;
            o.stiffness = stiffness == 1 ? WaveHoltzOptions::lobatto : WaveHoltzOptions::gauss;
            o.h_faces = h_faces;
            o.n_faces = n_faces;
            o.sweep = sweep == 1 ? WaveHoltzOptions::lattice : WaveHoltzOptions::operator_kernels;
            o.precision = precision == 1 ? WaveHoltzOptions::f32 : WaveHoltzOptions::f64;
            o.launch = launch == 1 ? WaveHoltzOptions::per_pair : WaveHoltzOptions::per_sweep;
            o.h_cell_stiffness = h_beta;
            auto h = new OpHandle;
            h->op.reset(new WaveHoltz(omega, h_a, *static_cast<H1Space *>(fem), o));
            return h;
        });
    }
    } // namespace
    namespace
    {
        const WaveHoltz &waveholtz_of(void *op)
        {
            auto *W = op ? dynamic_cast<const WaveHoltz *>(static_cast<OpHandle *>(op)->op.get()) : nullptr;
            if (!W)
                throw std::runtime_error("not a WaveHoltz operator");
            return *W;
        }
    } // namespace
    int cuddh_waveholtz_period(void *op, const double *z_in, const double *f, double *z_out)
    {
        return guarded([&] { waveholtz_of(op).period(z_in, f, z_out); });
    }
    int cuddh_waveholtz_solution(void *op, const double *z, double *u) { return guarded([&] { waveholtz_of(op).solution(z, u); }); }
    int cuddh_waveholtz_info(void *op, int *h_info, double *h_dt, char *kernel, int cap)
    {
        return guarded([&]
        {
            const WaveHoltz &W = waveholtz_of(op);
            if (h_info)
            {
                h_info[0] = W.num_steps();
                h_info[1] = W.time_ratio();
                h_info[2] = W.integrator().scheme == DDHIntegrator::rk4 ? 1 : 0;
                h_info[3] = W.integrator().coarsen;
                h_info[4] = W.sweeps_per_period();
                h_info[5] = W.size() / 2;
            }
            if (h_dt)
                *h_dt = W.time_step();
            if (kernel && cap > 0)
                std::snprintf(kernel, cap, "%s", W.stiffness_kernel().c_str());
        });
    }

    int cuddh_waveholtz_sweep(void *op)
    {
        int form = -1;
        guarded([&] { form = waveholtz_of(op).sweep() == WaveHoltzOptions::lattice ? 1 : 0; });
        return form;
    }
    int cuddh_waveholtz_precision(void *op)
    {
        int precision = -1;
        guarded([&] { precision = waveholtz_of(op).precision() == WaveHoltzOptions::f32 ? 1 : 0; });
        return precision;
    }
    int cuddh_waveholtz_launch(void *op)
    {
        int launch = -1;
        guarded([&] { launch = waveholtz_of(op).launch() == WaveHoltzOptions::per_pair ? 1 : 0; });
        return launch;
    }
    int cuddh_wave_lattice_map(void *fem, int *h_dims, double *h_h, int *h_node_of)
    {
        return guarded([&]
        {
            const WaveLatticeMap map = build_wave_lattice_map(*static_cast<H1Space *>(fem));
            const int dims[5] = {map.nx, map.ny, map.Lx, map.Ly, map.stride};
            if (h_dims)
                std::copy(dims, dims + 5, h_dims);
            if (h_h)
            {
                h_h[0] = map.hx;
                h_h[1] = map.hy;
            }
            if (h_node_of)
                std::copy(map.node_of.begin(), map.node_of.end(), h_node_of);
        });
    }
    int cuddh_wave_lattice_map_cells(void *fem, int *h_dims, double *h_h, int *h_node_of, unsigned char *h_cell)
    {
        return guarded([&]
        {
            const WaveLatticeMap map = build_wave_cells_map(*static_cast<H1Space *>(fem));
            const int dims[5] = {map.nx, map.ny, map.Lx, map.Ly, map.stride};
            if (h_dims)
                std::copy(dims, dims + 5, h_dims);
            if (h_h)
            {
                h_h[0] = map.hx;
                h_h[1] = map.hy;
            }
            if (h_node_of)
                std::copy(map.node_of.begin(), map.node_of.end(), h_node_of);
            if (h_cell)
                std::copy(map.cell.begin(), map.cell.end(), h_cell);
        });
    }
    int cuddh_wave_lattice_cell_weights(void *fem, const double *h_beta, double *h_weights, int *h_dims)
    {
        return guarded([&]
        {
            const H1Space &space = *static_cast<H1Space *>(fem);
            check_cell_stiffness(space.mesh().n_elem(), h_beta);
            const WaveLatticeMap map = build_wave_lattice_or_cells_map(space);
            const std::vector<double> weights = wave_lattice_cell_weights(map, space.mesh().n_elem(), h_beta);
            if (h_weights)
                std::copy(weights.begin(), weights.end(), h_weights);
            if (h_dims)
            {
                h_dims[0] = map.nx;
                h_dims[1] = map.ny;
            }
        });
    }
    int cuddh_waveholtz_coefficient_ratio(int n_elem, int nodes_per_elem, const int *h_I, const double *h_a, const double *h_beta, int *h_ratio)
    {
        return guarded([&]
        {
            if (h_beta)
                check_cell_stiffness(n_elem, h_beta);
            const int ratio = wave_coefficient_ratio(n_elem, nodes_per_elem, h_I, h_a, h_beta);
            if (h_ratio)
                *h_ratio = ratio;
        });
    }
    int cuddh_wave_lattice_tables(void *basis, double *h_A, double *h_w)
    {
        return guarded([&] { wave_lattice_tables(*static_cast<Basis *>(basis), h_A, h_w); });
    }

    // ------------------------------------------------------------ whole-domain WaveHoltz on a box (three dimensions)
    int cuddh_wave_box_describe(int nx, int ny, int nz, const double *h_box, int n_basis, const double *h_a, int face_mask, cuddh_wave_box *desc,
                                int *h_dims, double *h_m, double *h_h, double *h_invm, double *h_Hi, int *h_dof_of_slot, int *h_slot_of_dof)
    {
        return cuddh_wave_box_describe_rows(nx, ny, nz, h_box, n_basis, h_a, face_mask, 2, desc, h_dims, h_m, h_h, h_invm, h_Hi, h_dof_of_slot,
                                            h_slot_of_dof);
    }
    int cuddh_wave_box_describe_rows(int nx, int ny, int nz, const double *h_box, int n_basis, const double *h_a, int face_mask, int row_multiple,
                                     cuddh_wave_box *desc, int *h_dims, double *h_m, double *h_h, double *h_invm, double *h_Hi, int *h_dof_of_slot,
                                     int *h_slot_of_dof)
    {
        return guarded([&]
        {
            if (face_mask < 0)
                throw std::runtime_error("WaveHoltz error: box: the face mask has six bits (x0, x1, y0, y1, z0, z1), not " + std::to_string(face_mask) + ".");
            const WaveBox B = build_wave_box(nx, ny, nz, h_box, n_basis, h_a, static_cast<unsigned>(face_mask), row_multiple);
            if (desc)
                *desc = B.desc;
            if (h_dims)
            {
                h_dims[0] = B.Lx;
                h_dims[1] = B.Ly;
                h_dims[2] = B.Lz;
                h_dims[3] = B.desc.stride;
            }
            const std::pair<const std::vector<double> *, double *> reals[] = {{&B.m, h_m}, {&B.h, h_h}, {&B.invm, h_invm}, {&B.Hi, h_Hi}};
            for (const auto &r : reals)
                if (r.second)
                    std::copy(r.first->begin(), r.first->end(), r.second);
            if (h_dof_of_slot)
                std::copy(B.dof_of_slot.begin(), B.dof_of_slot.end(), h_dof_of_slot);
            if (h_slot_of_dof)
                std::copy(B.slot_of_dof.begin(), B.slot_of_dof.end(), h_slot_of_dof);
        });
    }
    namespace
    {
        // checked before anything else is looked at
        WaveHoltzBoxOptions box_options(const double *h_a, int integrator, int coarsen, int time_ratio, int face_mask, int precision = 0)
        {
            if (precision != 0 && precision != 1)
                throw std::runtime_error("WaveHoltz error: precision: the precision must be 0 (f64) or 1 (f32), not " + std::to_string(precision) + ".");
            if (integrator != 0 && integrator != 1)
                throw std::runtime_error("WaveHoltz error: integrator: the scheme must be 0 (rk2) or 1 (rk4), not " + std::to_string(integrator) + ".");
            if (face_mask < 0)
                throw std::runtime_error("WaveHoltz error: box: the face mask has six bits (x0, x1, y0, y1, z0, z1), not " + std::to_string(face_mask) + ".");
            if (!h_a)
                throw std::runtime_error("WaveHoltz error: box: no coefficient was given (NULL).");
            WaveHoltzBoxOptions o;
            o.integrator = {integrator == 1 ? DDHIntegrator::rk4 : DDHIntegrator::rk2, coarsen};
            o.time_ratio = time_ratio;
            o.faces = static_cast<unsigned>(face_mask);
            o.precision = precision == 1 ? WaveHoltzBoxOptions::f32 : WaveHoltzBoxOptions::f64;
            return o;
        }
    } // namespace
    int cuddh_waveholtz_box_time_grid(double omega, int nx, int ny, int nz, const double *h_box, int n_basis, const double *h_a, int integrator,
                                      int coarsen, int time_ratio, int face_mask, int *h_steps, double *h_dt)
    {
        return guarded([&]
        {
            const WaveBoxTimeGrid g = wave_box_time_grid(omega, nx, ny, nz, h_box, n_basis, h_a, box_options(h_a, integrator, coarsen, time_ratio, face_mask));
            if (h_steps)
            {
                h_steps[0] = g.nt;
                h_steps[1] = g.ratio;
            }
            if (h_dt)
                *h_dt = g.dt;
        });
    }
    void *cuddh_waveholtz_box_create(double omega, int nx, int ny, int nz, const double *h_box, int n_basis, const double *h_a, int integrator,
                                     int coarsen, int time_ratio, int face_mask)
    {
        return cuddh_waveholtz_box_create_precision(omega, nx, ny, nz, h_box, n_basis, h_a, integrator, coarsen, time_ratio, face_mask, 0);
    }
    void *cuddh_waveholtz_box_create_precision(double omega, int nx, int ny, int nz, const double *h_box, int n_basis, const double *h_a,
                                               int integrator, int coarsen, int time_ratio, int face_mask, int precision)
    {
        return guarded_new<OpHandle>([&]
        {
            const WaveHoltzBoxOptions o = box_options(h_a, integrator, coarsen, time_ratio, face_mask, precision);
            auto h = new OpHandle;
            try
            {
                h->op.reset(new WaveHoltzBox(omega, nx, ny, nz, h_box, n_basis, h_a, o));
            }
            catch (...)
            {
                delete h;
                throw;
            }
            return h;
        });
    }
    namespace
    {
        const WaveHoltzBox &waveholtz_box_of(void *op)
        {
            auto *W = op ? dynamic_cast<const WaveHoltzBox *>(static_cast<OpHandle *>(op)->op.get()) : nullptr;
            if (!W)
                throw std::runtime_error("not a WaveHoltzBox operator");
            return *W;
        }
    } // namespace
    int cuddh_waveholtz_box_period(void *op, const double *z_in, const double *f, double *z_out)
    {
        return guarded([&] { waveholtz_box_of(op).period(z_in, f, z_out); });
    }
    int cuddh_waveholtz_box_solution(void *op, const double *z, double *u) { return guarded([&] { waveholtz_box_of(op).solution(z, u); }); }
    int cuddh_waveholtz_box_info(void *op, int *h_info, double *h_dt, char *kernel, int cap)
    {
        return guarded([&]
        {
            const WaveHoltzBox &W = waveholtz_box_of(op);
            if (h_info)
            {
                h_info[0] = W.num_steps();
                h_info[1] = W.time_ratio();
                h_info[2] = W.integrator().scheme == DDHIntegrator::rk4 ? 1 : 0;
                h_info[3] = W.integrator().coarsen;
                h_info[4] = W.sweeps_per_period();
                h_info[5] = W.size() / 2;
            }
            if (h_dt)
                *h_dt = W.time_step();
            if (kernel && cap > 0)
                std::snprintf(kernel, cap, "%s", W.stiffness_kernel().c_str());
        });
    }
    int cuddh_waveholtz_box_lattice(void *op, int *h_dims)
    {
        return guarded([&] { waveholtz_box_of(op).lattice(h_dims); });
    }
    int cuddh_waveholtz_box_precision(void *op)
    {
        int code = -1;
        guarded([&] { code = waveholtz_box_of(op).precision() == WaveHoltzBoxOptions::f32 ? 1 : 0; });
        return code;
    }

    int cuddh_helmholtz_read_stamps(void *op, unsigned long long *h_out, int n_patches)
    {
        auto *h = static_cast<OpHandle *>(op);
        if (!h->helm)
            return -1;
        return cuddh_hip_helmholtz_plan_read_stamps(h->helm->kernel_plan(), h_out, n_patches);
    }
    size_t cuddh_helmholtz_bytes(void *op, int actual)
    {
        auto *h = static_cast<OpHandle *>(op);
        if (!h->helm)
            return 0;
        return actual == 3 ? h->helm->bytes_native() : (actual == 2 ? h->helm->bytes_affine() : h->helm->bytes_per_apply(actual != 0));
    }
    int cuddh_helmholtz_has_native(void *op)
    {
        auto *h = static_cast<OpHandle *>(op);
        return h->helm && h->helm->has_native() ? 1 : 0;
    }
    static HelmholtzOperator &helm_of(void *op)
    {
        auto *h = static_cast<OpHandle *>(op);
        if (!h->helm)
            throw std::runtime_error("not a Helmholtz operator");
        return *h->helm;
    }
    int cuddh_helmholtz_to_native(void *op, const double *x, double *z) { return guarded([&] { helm_of(op).to_native(x, z); }); }
    int cuddh_helmholtz_from_native(void *op, const double *z, double *y) { return guarded([&] { helm_of(op).from_native(z, y); }); }
    int cuddh_helmholtz_apply_native(void *op, const double *z_in, double *z_out) { return guarded([&] { helm_of(op).action_native(z_in, z_out); }); }

    // ------------------------------------------------------------ functionals
    int cuddh_linear_functional(void *fem, int nq, int integrand, double param, double c, int accumulate, double *F)
    {
        return guarded([&]
        {
            const H1Space &f = *static_cast<H1Space *>(fem);
            const Integrand g{integrand, param};
            if (nq > 0)
            {
                LinearFunctional l(f, QuadratureRule(nq, QuadratureRule::GaussLegendre));
                if (!accumulate)
                    zeros(f.size(), F);
                l.action(c, g, F);
                detail::check_hip(cuddh_hip_stream_sync(stream()), "linear functional"); // scratch dies with l
            }
            else
            {
                LinearFunctional l(f);
                if (!accumulate)
                    zeros(f.size(), F);
                l.action(c, g, F);
                detail::check_hip(cuddh_hip_stream_sync(stream()), "linear functional");
            }
        });
    }
    int cuddh_face_linear_functional(void *fs_, int nq, int integrand, double param, double c, int accumulate, double *F)
    {
        return guarded([&]
        {
            const FaceSpace &fs = *static_cast<FaceSpace *>(fs_);
            const Integrand g{integrand, param};
            if (nq > 0)
            {
                FaceLinearFunctional l(fs, QuadratureRule(nq, QuadratureRule::GaussLegendre));
                if (!accumulate)
                    zeros(fs.size(), F);
                l.action(c, g, F);
                detail::check_hip(cuddh_hip_stream_sync(stream()), "face linear functional");
            }
            else
            {
                FaceLinearFunctional l(fs);
                if (!accumulate)
                    zeros(fs.size(), F);
                l.action(c, g, F);
                detail::check_hip(cuddh_hip_stream_sync(stream()), "face linear functional");
            }
        });
    }
    int cuddh_nodal_values(void *fem, int integrand, double param, double *out)
    {
        return guarded([&]
        {
            const H1Space &f = *static_cast<H1Space *>(fem);
            const double *X = f.physical_coordinates(MemorySpace::DEVICE);
            const Integrand g{integrand, param};
            forall(f.size(), [=] __device__(int i) -> void
            {
                const double xy[2] = {X[2 * i], X[2 * i + 1]};
                out[i] = g(xy);
            });
        });
    }

    // ------------------------------------------------------------ DDH
    void *cuddh_ddh_create(double omega, const double *h_a, void *fem, int nx, int ny, int f64, int kernel)
    {
        return guarded_new<DdhHandle>([&]
        {
            auto h = new DdhHandle;
            const H1Space &f = *static_cast<H1Space *>(fem);
            if (f64)
                h->f64.reset(new DDH64(omega, h_a, f, nx, ny, kernel));
            else
                h->f32.reset(new DDH(omega, h_a, f, nx, ny, kernel));
            return h;
        });
    }
    void *cuddh_ddh_create_block(double omega, const double *h_a, void *fem, int nx, int ny, int block, int f64, int kernel)
    {
        return guarded_new<DdhHandle>([&]
        {
            auto h = new DdhHandle;
            const H1Space &f = *static_cast<H1Space *>(fem);
            try
            {
                if (f64)
                    h->f64.reset(new DDH64(omega, h_a, f, nx, ny, kernel, block));
                else
                    h->f32.reset(new DDH(omega, h_a, f, nx, ny, kernel, block));
            }
            catch (...)
            {
                delete h;
                throw;
            }
            return h;
        });
    }
    void *cuddh_ddh_create_labels(double omega, const double *h_a, void *fem, int n_domains, const int *h_labels, int f64, int kernel)
    {
        return guarded_new<DdhHandle>([&]
        {
            auto h = new DdhHandle;
            const H1Space &f = *static_cast<H1Space *>(fem);
            try
            {
                if (f64)
                    h->f64.reset(new DDH64(from_labels, omega, h_a, f, n_domains, h_labels, kernel));
                else
                    h->f32.reset(new DDH(from_labels, omega, h_a, f, n_domains, h_labels, kernel));
            }
            catch (...)
            {
                delete h;
                throw;
            }
            return h;
        });
    }
    void *cuddh_ddh_create_labels_integrator(double omega, const double *h_a, void *fem, int n_domains, const int *h_labels, int f64, int kernel,
                                             int policy, const int *h_ratios, int n_ratios, int integrator, int coarsen)
    {
        return guarded_new<DdhHandle>([&]
        {
            if (integrator < 0 || integrator > 1)
                cuddh_error("DDH error: integrator: must be 0 (rk2) or 1 (rk4).");
            if (policy < 0 || policy > 2)
                cuddh_error("DDH error: time step: policy must be 0 (mesh), 1 (coefficient) or 2 (ratios).");
            const DDHTimeStep ts = policy == 2   ? DDHTimeStep::from_ratios(h_ratios, n_ratios)
                                   : policy == 1 ? DDHTimeStep::from_coefficient()
                                                 : DDHTimeStep::from_mesh();
            DDHIntegrator ig;
            ig.scheme = integrator == 1 ? DDHIntegrator::rk4 : DDHIntegrator::rk2;
            ig.coarsen = coarsen;
            auto h = new DdhHandle;
            const H1Space &f = *static_cast<H1Space *>(fem);
            try
            {
                if (f64)
                    h->f64.reset(new DDH64(from_labels, omega, h_a, f, n_domains, h_labels, kernel, ts, ig));
                else
                    h->f32.reset(new DDH(from_labels, omega, h_a, f, n_domains, h_labels, kernel, ts, ig));
            }
            catch (...)
            {
                delete h;
                throw;
            }
            return h;
        });
    }
    void *cuddh_ddh_create_timegrid(double omega, const double *h_a, void *fem, int nx, int ny, int block, int f64, int kernel, int policy,
                                    const int *h_ratios, int n_ratios)
    {
        return guarded_new<DdhHandle>([&]
        {
            if (policy < 0 || policy > 2)
                cuddh_error("DDH error: time step: policy must be 0 (mesh), 1 (coefficient) or 2 (ratios).");
            const DDHTimeStep ts = policy == 2   ? DDHTimeStep::from_ratios(h_ratios, n_ratios)
                                   : policy == 1 ? DDHTimeStep::from_coefficient()
                                                 : DDHTimeStep::from_mesh();
            auto h = new DdhHandle;
            const H1Space &f = *static_cast<H1Space *>(fem);
            try
            {
                if (f64)
                    h->f64.reset(new DDH64(omega, h_a, f, nx, ny, kernel, block, ts));
                else
                    h->f32.reset(new DDH(omega, h_a, f, nx, ny, kernel, block, ts));
            }
            catch (...)
            {
                delete h;
                throw;
            }
            return h;
        });
    }
    void *cuddh_ddh_create_integrator(double omega, const double *h_a, void *fem, int nx, int ny, int block, int f64, int kernel, int policy,
                                      const int *h_ratios, int n_ratios, int integrator, int coarsen)
    {
        return guarded_new<DdhHandle>([&]
        {
            if (integrator < 0 || integrator > 1)
                cuddh_error("DDH error: integrator: must be 0 (rk2) or 1 (rk4).");
            if (policy < 0 || policy > 2)
                cuddh_error("DDH error: time step: policy must be 0 (mesh), 1 (coefficient) or 2 (ratios).");
            const DDHTimeStep ts = policy == 2   ? DDHTimeStep::from_ratios(h_ratios, n_ratios)
                                   : policy == 1 ? DDHTimeStep::from_coefficient()
                                                 : DDHTimeStep::from_mesh();
            DDHIntegrator ig;
            ig.scheme = integrator == 1 ? DDHIntegrator::rk4 : DDHIntegrator::rk2;
            ig.coarsen = coarsen;
            auto h = new DdhHandle;
            const H1Space &f = *static_cast<H1Space *>(fem);
            try
            {
                if (f64)
                    h->f64.reset(new DDH64(omega, h_a, f, nx, ny, kernel, block, ts, ig));
                else
                    h->f32.reset(new DDH(omega, h_a, f, nx, ny, kernel, block, ts, ig));
            }
            catch (...)
            {
                delete h;
                throw;
            }
            return h;
        });
    }
    int cuddh_ddh_integrator(void *d, int *scheme, int *coarsen)
    {
        return guarded([&]
        {
            auto *h = static_cast<DdhHandle *>(d);
            const DDHIntegrator ig = h->is64() ? h->f64->internals().integrator() : h->f32->internals().integrator();
            if (scheme)
                *scheme = ig.scheme == DDHIntegrator::rk4 ? 1 : 0;
            if (coarsen)
                *coarsen = ig.coarsen;
        });
    }
    int cuddh_ddh_time_ratios(void *d, int *h_out)
    {
        int n = -1;
        guarded([&]
        {
            auto *h = static_cast<DdhHandle *>(d);
            const std::vector<int> &r = h->is64() ? h->f64->internals().time_ratios() : h->f32->internals().time_ratios();
            if (h_out)
                std::copy(r.begin(), r.end(), h_out);
            n = static_cast<int>(r.size());
        });
        return n;
    }
    void cuddh_ddh_destroy(void *d) { delete static_cast<DdhHandle *>(d); }
    int cuddh_ddh_size(void *d)
    {
        auto *h = static_cast<DdhHandle *>(d);
        return h->is64() ? h->f64->size() : h->f32->size();
    }
    int cuddh_ddh_info(void *d, int *info, double *h_dt)
    {
        return guarded([&]
        {
            auto *h = static_cast<DdhHandle *>(d);
            auto fill = [&](const auto &c)
            {
                info[0] = c.num_domains();
                info[1] = c.num_steps();
                info[2] = c.n_traces() / 2;
                info[3] = c.max_dof();
                info[4] = c.max_fdof();
                info[5] = c.elems_per_side();
                info[6] = cuddh_hip_device_count() > 0 ? c.kernel_kind() : -1;
                *h_dt = c.time_step();
            };
            if (h->is64())
                fill(h->f64->internals());
            else
                fill(h->f32->internals());
            info[7] = h->is64() ? 1 : 0;
        });
    }
    int cuddh_ddh_solve_multi_gpu(int nx, int nb, double omega, const double *h_a, const double *h_f, double *h_u, int world, int m,
                                  int maxit, double tol, int force_rccl, cuddh_multi_gpu_result *out, double *h_res)
    {
        return guarded([&]
        {
            const multi_gpu_result r = ddh_solve_multi_gpu(nx, nb, omega, h_a, h_f, h_u, world, m, maxit, static_cast<float>(tol), force_rccl & 3,
                                                           (force_rccl & 4) != 0, (force_rccl >> 8) & 0xFF, (force_rccl >> 16) & 0xFF);
            out->success = r.gmres.success ? 1 : 0;
            out->num_iter = r.gmres.num_iter;
            out->num_matvec = r.gmres.num_matvec;
            out->n_res = static_cast<int>(r.gmres.res_norm.size());
            out->world = r.world;
            out->used_rccl = r.used_rccl ? 1 : 0;
            out->t_setup = r.t_setup;
            out->t_rhs = r.t_rhs;
            out->t_gmres = r.t_gmres;
            out->t_postprocess = r.t_postprocess;
            out->bytes_sent_per_action_rank0 = r.bytes_sent_per_action_rank0;
            for (int i = 0; i < out->n_res && i < maxit + 2; ++i)
                h_res[i] = r.gmres.res_norm[i];
        });
    }
    int cuddh_helmholtz_multi_gpu(void *mesh, int nb, double omega, const double *h_a2x, const double *h_ax, const double *h_x, double *h_y,
                                  int world, int transport, int reps, int m, int maxit, double tol, cuddh_helmholtz_multi_gpu_result *out, double *h_res)
    {
        return guarded([&]
        {
            const QuadMeshData g = mesh_data(*static_cast<Mesh2D *>(mesh));
            const helmholtz_multi_gpu_result r = helmholtz_multi_gpu(g.n_pts(), g.xy.data(), g.n_elem(), g.elems.data(), nb, omega, h_a2x, h_ax, h_x, h_y,
                                                                     world, transport, reps, m, maxit, tol);
            out->success = r.gmres.success ? 1 : 0;
            out->num_iter = r.gmres.num_iter;
            out->num_matvec = r.gmres.num_matvec;
            out->n_res = static_cast<int>(r.gmres.res_norm.size());
            out->world = r.world;
            out->used_rccl = r.used_rccl ? 1 : 0;
            out->t_setup = r.t_setup;
            out->t_apply = r.t_apply;
            out->t_gmres = r.t_gmres;
            out->n_loc_max = r.n_loc_max;
            out->n_halo_max = r.n_halo_max;
            out->halo_bytes_per_apply_max = r.halo_bytes_per_apply_max;
            for (int i = 0; h_res && i < out->n_res && i < maxit + 2; ++i)
                h_res[i] = r.gmres.res_norm[i];
        });
    }
    int cuddh_helmholtz_partition_query(void *mesh, void *fem, void *fs, int rank, int world, int which, int peer, int *h_out)
    {
        int count = -1;
        const int err = guarded([&]
        {
            const H1Space &f = *static_cast<H1Space *>(fem);
            const HelmholtzPartition p = HelmholtzPartition::build(*static_cast<Mesh2D *>(mesh), f.basis(), f, *static_cast<FaceSpace *>(fs), rank, world);
            static const std::vector<int> none;
            const std::vector<int> *v = &none;
            if (which == 0)
                v = &p.my_elems;
            else if (which == 1)
                v = &p.l2g;
            else if (which == 2)
                v = &p.owned;
            else if (which == 3)
                v = &p.halo;
            else if (which == 4 || which == 5)
            {
                const auto &m = which == 4 ? p.own_to : p.halo_from;
                const auto it = m.find(peer);
                if (it != m.end())
                    v = &it->second;
            }
            else if (which == 6)
                v = &p.face_l2g;
            else if (which == 7)
                v = &p.faces;
            count = static_cast<int>(v->size());
            if (h_out)
                std::copy(v->begin(), v->end(), h_out);
        });
        return err ? -1 : count;
    }
    int cuddh_trace_exchange_query(const int *h_B, int n_domains, int mx_fdof, int n_lambda, int rank, int world, int which, int peer,
                                   int *h_out)
    {
        int count = -1;
        const int err = guarded([&]
        {
            const TraceExchangePlan p = TraceExchangePlan::build(h_B, n_domains, mx_fdof, n_lambda, rank, world);
            const std::vector<int> *v = nullptr;
            static const std::vector<int> none;
            if (which == 0)
                v = &p.owned;
            else if (which == 3)
                v = &p.boundary;
            else if (which == 4)
                v = &p.interior;
            else
            {
                const auto &m = which == 1 ? p.send : p.recv;
                const auto it = m.find(peer);
                v = it == m.end() ? &none : &it->second;
            }
            count = static_cast<int>(v->size());
            if (h_out)
                std::copy(v->begin(), v->end(), h_out);
        });
        return err ? -1 : count;
    }
    int cuddh_ddh_set_wh_iters(void *d, int n)
    {
        return guarded([&]
        {
            auto *h = static_cast<DdhHandle *>(d);
            if (h->is64())
                h->f64->internals().set_waveholtz_iterations(n);
            else
                h->f32->internals().set_waveholtz_iterations(n);
        });
    }
    int cuddh_ddh_set_wave_priority(void *d, int high)
    {
        return guarded([&]
        {
            auto *h = static_cast<DdhHandle *>(d);
            if (h->is64())
                h->f64->internals().set_wave_priority(high != 0);
            else
                h->f32->internals().set_wave_priority(high != 0);
        });
    }
    int cuddh_ddh_set_sweep_form(void *d, int form)
    {
        return guarded([&]
        {
            auto *h = static_cast<DdhHandle *>(d);
            if (h->is64())
                h->f64->internals().set_sweep_form(form);
            else
                h->f32->internals().set_sweep_form(form);
        });
    }
    int cuddh_ddh_set_chain_order(void *d, int order)
    {
        return guarded([&]
        {
            auto *h = static_cast<DdhHandle *>(d);
            if (h->is64())
                h->f64->internals().set_chain_order(order);
            else
                h->f32->internals().set_chain_order(order);
        });
    }
    int cuddh_ddh_chain_order(void *d)
    {
        int order = 0;
        const int err = guarded([&]
        {
            auto *h = static_cast<DdhHandle *>(d);
            order = h->is64() ? h->f64->internals().chain_order() : h->f32->internals().chain_order();
        });
        return err ? -1 : order;
    }
    int cuddh_ddh_set_forcing(void *d, int forcing)
    {
        return guarded([&]
        {
            auto *h = static_cast<DdhHandle *>(d);
            if (h->is64())
                h->f64->internals().set_forcing(forcing);
            else
                h->f32->internals().set_forcing(forcing);
        });
    }
    int cuddh_ddh_forcing(void *d)
    {
        int forcing = 0;
        const int err = guarded([&]
        {
            auto *h = static_cast<DdhHandle *>(d);
            forcing = h->is64() ? h->f64->internals().forcing() : h->f32->internals().forcing();
        });
        return err ? -1 : forcing;
    }
    int cuddh_ddh_set_march(void *d, int march)
    {
        return guarded([&]
        {
            auto *h = static_cast<DdhHandle *>(d);
            if (h->is64())
                h->f64->internals().set_march(march);
            else
                h->f32->internals().set_march(march);
        });
    }
    int cuddh_ddh_march(void *d)
    {
        int march = 0;
        const int err = guarded([&]
        {
            auto *h = static_cast<DdhHandle *>(d);
            march = h->is64() ? h->f64->internals().march() : h->f32->internals().march();
        });
        return err ? -1 : march;
    }
    int cuddh_ddh_set_head(void *d, int head)
    {
        return guarded([&]
        {
            auto *h = static_cast<DdhHandle *>(d);
            if (h->is64())
                h->f64->internals().set_head(head);
            else
                h->f32->internals().set_head(head);
        });
    }
    int cuddh_ddh_head(void *d)
    {
        int head = 0;
        const int err = guarded([&]
        {
            auto *h = static_cast<DdhHandle *>(d);
            head = h->is64() ? h->f64->internals().head() : h->f32->internals().head();
        });
        return err ? -1 : head;
    }
    int cuddh_ddh_set_assembly(void *d, int assembly)
    {
        return guarded([&]
        {
            auto *h = static_cast<DdhHandle *>(d);
            if (h->is64())
                h->f64->internals().set_assembly(assembly);
            else
                h->f32->internals().set_assembly(assembly);
        });
    }
    int cuddh_ddh_assembly(void *d)
    {
        int assembly = 0;
        const int err = guarded([&]
        {
            auto *h = static_cast<DdhHandle *>(d);
            assembly = h->is64() ? h->f64->internals().assembly() : h->f32->internals().assembly();
        });
        return err ? -1 : assembly;
    }
    int cuddh_ddh_set_owner_rule(void *d, int last)
    {
        return guarded([&]
        {
            auto *h = static_cast<DdhHandle *>(d);
            if (h->is64())
                h->f64->internals().set_last_copy_publishes(last != 0);
            else
                h->f32->internals().set_last_copy_publishes(last != 0);
        });
    }
    int cuddh_ddh_sweep_form(void *d)
    {
        int form = 0;
        const int err = guarded([&]
        {
            auto *h = static_cast<DdhHandle *>(d);
            form = h->is64() ? h->f64->internals().sweep_form() : h->f32->internals().sweep_form();
        });
        return err ? -1 : form;
    }
    int cuddh_ddh_rhs(void *d, const double *f, void *b)
    {
        return guarded([&]
        {
            auto *h = static_cast<DdhHandle *>(d);
            if (h->is64())
                h->f64->rhs(f, static_cast<double *>(b));
            else
                h->f32->rhs(f, static_cast<float *>(b));
        });
    }
    int cuddh_ddh_postprocess(void *d, const void *lambda, const double *f, double *u)
    {
        return guarded([&]
        {
            auto *h = static_cast<DdhHandle *>(d);
            if (h->is64())
                h->f64->postprocess(static_cast<const double *>(lambda), f, u);
            else
                h->f32->postprocess(static_cast<const float *>(lambda), f, u);
        });
    }
    int cuddh_ddh_action(void *d, const void *x, void *y)
    {
        return guarded([&]
        {
            auto *h = static_cast<DdhHandle *>(d);
            if (h->is64())
                h->f64->action(static_cast<const double *>(x), static_cast<double *>(y));
            else
                h->f32->action(static_cast<const float *>(x), static_cast<float *>(y));
        });
    }
    int cuddh_ddh_local_traces(void *d, int d0, int d1, const double *f, const void *lambda, void *update)
    {
        return guarded([&]
        {
            auto *h = static_cast<DdhHandle *>(d);
            if (h->is64())
                h->f64->local_traces(d0, d1, f, static_cast<const double *>(lambda), static_cast<double *>(update));
            else
                h->f32->local_traces(d0, d1, f, static_cast<const float *>(lambda), static_cast<float *>(update));
        });
    }
    int cuddh_ddh_local_traces_listed(void *d, const int *d_domains, int n, const double *f, const void *lambda, void *update)
    {
        return guarded([&]
        {
            auto *h = static_cast<DdhHandle *>(d);
            if (h->is64())
                h->f64->internals().solve_listed(d_domains, n, f, static_cast<const double *>(lambda), static_cast<double *>(update));
            else
                h->f32->internals().solve_listed(d_domains, n, f, static_cast<const float *>(lambda), static_cast<float *>(update));
        });
    }
    int cuddh_ddh_local_solution_listed(void *d, const int *d_domains, int n, const void *lambda, const double *f, double *u, int zero_u)
    {
        return guarded([&]
        {
            auto *h = static_cast<DdhHandle *>(d);
            if (h->is64())
                h->f64->internals().solve_listed(d_domains, n, f, u, zero_u != 0, static_cast<const double *>(lambda), nullptr);
            else
                h->f32->internals().solve_listed(d_domains, n, f, u, zero_u != 0, static_cast<const float *>(lambda), nullptr);
        });
    }
    int cuddh_ddh_local_solution(void *d, int d0, int d1, const void *lambda, const double *f, double *u, int zero_u)
    {
        return guarded([&]
        {
            auto *h = static_cast<DdhHandle *>(d);
            if (h->is64())
                h->f64->local_solution(d0, d1, static_cast<const double *>(lambda), f, u, zero_u != 0);
            else
                h->f32->local_solution(d0, d1, static_cast<const float *>(lambda), f, u, zero_u != 0);
        });
    }
    long long cuddh_ddh_table(void *d, const char *name, void *h_out, int count_only)
    {
        long long n = -1;
        guarded([&]
        {
            auto *h = static_cast<DdhHandle *>(d);
            n = h->is64() ? ddh_table(h->f64->internals(), name, h_out, count_only) : ddh_table(h->f32->internals(), name, h_out, count_only);
        });
        return n;
    }

    // ------------------------------------------------------------ GMRES
    // One core per kind of operator.  The entry points spell the options of krylov.hpp (GmresOptions) differently: none, `_orth`
    // (0 mgs, 1 cgs2), `_aug` (orth, and augment = k: LGMRES), `_cplx` (complex arithmetic on split [Re; Im] vectors).  The
    // options are checked as the arguments of the core's call, inside guarded and before anything touches the device.
    static void gmres_operator(int n, double *x, void *op, const double *b, void *precond, int m, int maxit, double tol, int verbose, double max_seconds,
                               const GmresOptions &opt, cuddh_solver_result *out, double *h_res, double *h_time)
    {
        const Operator *A = static_cast<OpHandle *>(op)->op.get();
        fill_result(precond ? gmres(n, x, A, b, static_cast<OpHandle *>(precond)->op.get(), m, maxit, tol, verbose, max_seconds, opt)
                            : gmres(n, x, A, b, m, maxit, tol, verbose, max_seconds, opt),
                    out, h_res, h_time);
    }

    static void gmres_helmholtz(void *op, double *x, const double *b, int m, int maxit, double tol, int verbose, double max_seconds, const GmresOptions &opt,
                                cuddh_solver_result *out, double *h_res, double *h_time)
    {
        fill_result(helm_of(op).gmres(x, b, m, maxit, tol, verbose, max_seconds, opt), out, h_res, h_time);
    }

    static void gmres_ddh(int n, void *x, void *ddh, const void *b, int m, int maxit, double tol, int verbose, double max_seconds, const GmresOptions &opt,
                          cuddh_solver_result *out, double *h_res, double *h_time)
    {
        auto *h = static_cast<DdhHandle *>(ddh);
        fill_result(h->is64() ? gmres(n, static_cast<double *>(x), h->f64.get(), static_cast<const double *>(b), m, maxit, tol, verbose, max_seconds, opt)
                              : gmres(n, static_cast<float *>(x), h->f32.get(), static_cast<const float *>(b), m, maxit, static_cast<float>(tol), verbose,
                                      max_seconds, opt),
                    out, h_res, h_time);
    }

    // reduce: null, or the sum over the ranks of partitioned vectors
    static void gmres_callback(int n, void *x, cuddh_action_cb cb, void *ctx, const ScalarReduce *reduce, const void *b, int is_f64, int m, int maxit, double tol,
                               int verbose, double max_seconds, const GmresOptions &opt, cuddh_solver_result *out, double *h_res, double *h_time)
    {
        solver_out o;
        if (is_f64)
        {
            CallbackOp64 A(cb, ctx);
            double *x64 = static_cast<double *>(x);
            const double *b64 = static_cast<const double *>(b);
            o = reduce ? gmres(n, x64, &A, b64, m, maxit, tol, verbose, max_seconds, *reduce, opt) : gmres(n, x64, &A, b64, m, maxit, tol, verbose, max_seconds, opt);
        }
        else
        {
            CallbackOp32 A(cb, ctx);
            float *x32 = static_cast<float *>(x);
            const float *b32 = static_cast<const float *>(b);
            const float tol32 = static_cast<float>(tol);
            o = reduce ? gmres(n, x32, &A, b32, m, maxit, tol32, verbose, max_seconds, *reduce, opt) : gmres(n, x32, &A, b32, m, maxit, tol32, verbose, max_seconds, opt);
        }
        fill_result(o, out, h_res, h_time);
    }

    static void gmres_callback_sharded(int n, void *x, cuddh_action_cb cb, void *ctx, cuddh_reduce_cb reduce, void *reduce_ctx, const void *b, int is_f64, int m,
                                       int maxit, double tol, int verbose, double max_seconds, const GmresOptions &opt, cuddh_solver_result *out, double *h_res,
                                       double *h_time)
    {
        const ScalarReduce red{reduce, reduce_ctx};
        gmres_callback(n, x, cb, ctx, &red, b, is_f64, m, maxit, tol, verbose, max_seconds, opt, out, h_res, h_time);
    }

    int cuddh_gmres_f64(int n, double *x, void *op, const double *b, void *precond, int m, int maxit, double tol, int verbose,
                        double max_seconds, cuddh_solver_result *out, double *h_res, double *h_time)
    {
        return guarded([&] { gmres_operator(n, x, op, b, precond, m, maxit, tol, verbose, max_seconds, GmresOptions(), out, h_res, h_time); });
    }
    int cuddh_gmres_helmholtz(void *op, double *x, const double *b, int m, int maxit, double tol, int verbose, double max_seconds,
                              cuddh_solver_result *out, double *h_res, double *h_time)
    {
        return guarded([&] { gmres_helmholtz(op, x, b, m, maxit, tol, verbose, max_seconds, GmresOptions(), out, h_res, h_time); });
    }
    int cuddh_gmres_ddh(int n, void *x, void *ddh, const void *b, int m, int maxit, double tol, int verbose, double max_seconds,
                        cuddh_solver_result *out, double *h_res, double *h_time)
    {
        return guarded([&] { gmres_ddh(n, x, ddh, b, m, maxit, tol, verbose, max_seconds, GmresOptions(), out, h_res, h_time); });
    }
    int cuddh_gmres_callback(int n, void *x, cuddh_action_cb cb, void *ctx, const void *b, int is_f64, int m, int maxit, double tol,
                             int verbose, double max_seconds, cuddh_solver_result *out, double *h_res, double *h_time)
    {
        return guarded([&] { gmres_callback(n, x, cb, ctx, nullptr, b, is_f64, m, maxit, tol, verbose, max_seconds, GmresOptions(), out, h_res, h_time); });
    }
    int cuddh_gmres_callback_sharded(int n, void *x, cuddh_action_cb cb, void *ctx, cuddh_reduce_cb reduce, void *reduce_ctx,
                                     const void *b, int is_f64, int m, int maxit, double tol, int verbose, double max_seconds,
                                     cuddh_solver_result *out, double *h_res, double *h_time)
    {
        return guarded([&] { gmres_callback_sharded(n, x, cb, ctx, reduce, reduce_ctx, b, is_f64, m, maxit, tol, verbose, max_seconds, GmresOptions(), out, h_res, h_time); });
    }

    // ---- a chosen orthogonalisation (0 mgs, 1 cgs2)
    int cuddh_gmres_f64_orth(int n, double *x, void *op, const double *b, void *precond, int m, int maxit, double tol, int verbose,
                             double max_seconds, int orth, cuddh_solver_result *out, double *h_res, double *h_time)
    {
        return guarded([&] { gmres_operator(n, x, op, b, precond, m, maxit, tol, verbose, max_seconds, GmresOptions{orth_of(orth)}, out, h_res, h_time); });
    }
    int cuddh_gmres_helmholtz_orth(void *op, double *x, const double *b, int m, int maxit, double tol, int verbose, double max_seconds,
                                   int orth, cuddh_solver_result *out, double *h_res, double *h_time)
    {
        return guarded([&] { gmres_helmholtz(op, x, b, m, maxit, tol, verbose, max_seconds, GmresOptions{orth_of(orth)}, out, h_res, h_time); });
    }
    int cuddh_gmres_ddh_orth(int n, void *x, void *ddh, const void *b, int m, int maxit, double tol, int verbose, double max_seconds,
                             int orth, cuddh_solver_result *out, double *h_res, double *h_time)
    {
        return guarded([&] { gmres_ddh(n, x, ddh, b, m, maxit, tol, verbose, max_seconds, GmresOptions{orth_of(orth)}, out, h_res, h_time); });
    }
    int cuddh_gmres_callback_orth(int n, void *x, cuddh_action_cb cb, void *ctx, const void *b, int is_f64, int m, int maxit, double tol,
                                  int verbose, double max_seconds, int orth, cuddh_solver_result *out, double *h_res, double *h_time)
    {
        return guarded([&] { gmres_callback(n, x, cb, ctx, nullptr, b, is_f64, m, maxit, tol, verbose, max_seconds, GmresOptions{orth_of(orth)}, out, h_res, h_time); });
    }
    int cuddh_gmres_callback_sharded_orth(int n, void *x, cuddh_action_cb cb, void *ctx, cuddh_reduce_cb reduce, void *reduce_ctx,
                                          const void *b, int is_f64, int m, int maxit, double tol, int verbose, double max_seconds,
                                          int orth, cuddh_solver_result *out, double *h_res, double *h_time)
    {
        return guarded([&] { gmres_callback_sharded(n, x, cb, ctx, reduce, reduce_ctx, b, is_f64, m, maxit, tol, verbose, max_seconds, GmresOptions{orth_of(orth)}, out, h_res, h_time); });
    }

    // ---- orthogonalisation and augmentation chosen (augment = k: LGMRES)
    int cuddh_gmres_f64_aug(int n, double *x, void *op, const double *b, void *precond, int m, int maxit, double tol, int verbose,
                            double max_seconds, int orth, int augment, cuddh_solver_result *out, double *h_res, double *h_time)
    {
        return guarded([&] { gmres_operator(n, x, op, b, precond, m, maxit, tol, verbose, max_seconds, options_of(orth, augment, m), out, h_res, h_time); });
    }
    int cuddh_gmres_helmholtz_aug(void *op, double *x, const double *b, int m, int maxit, double tol, int verbose, double max_seconds,
                                  int orth, int augment, cuddh_solver_result *out, double *h_res, double *h_time)
    {
        return guarded([&] { gmres_helmholtz(op, x, b, m, maxit, tol, verbose, max_seconds, options_of(orth, augment, m), out, h_res, h_time); });
    }
    int cuddh_gmres_ddh_aug(int n, void *x, void *ddh, const void *b, int m, int maxit, double tol, int verbose, double max_seconds,
                            int orth, int augment, cuddh_solver_result *out, double *h_res, double *h_time)
    {
        return guarded([&] { gmres_ddh(n, x, ddh, b, m, maxit, tol, verbose, max_seconds, options_of(orth, augment, m), out, h_res, h_time); });
    }
    int cuddh_gmres_callback_aug(int n, void *x, cuddh_action_cb cb, void *ctx, const void *b, int is_f64, int m, int maxit, double tol,
                                 int verbose, double max_seconds, int orth, int augment, cuddh_solver_result *out, double *h_res, double *h_time)
    {
        return guarded([&] { gmres_callback(n, x, cb, ctx, nullptr, b, is_f64, m, maxit, tol, verbose, max_seconds, options_of(orth, augment, m), out, h_res, h_time); });
    }
    int cuddh_gmres_callback_sharded_aug(int n, void *x, cuddh_action_cb cb, void *ctx, cuddh_reduce_cb reduce, void *reduce_ctx,
                                         const void *b, int is_f64, int m, int maxit, double tol, int verbose, double max_seconds,
                                         int orth, int augment, cuddh_solver_result *out, double *h_res, double *h_time)
    {
        return guarded([&] { gmres_callback_sharded(n, x, cb, ctx, reduce, reduce_ctx, b, is_f64, m, maxit, tol, verbose, max_seconds, options_of(orth, augment, m), out, h_res, h_time); });
    }

    // ---- over the complex numbers on split [Re; Im] vectors (krylov.hpp: Arithmetic::complex)
    int cuddh_gmres_ddh_cplx(int n, void *x, void *ddh, const void *b, int m, int maxit, double tol, int verbose, double max_seconds,
                             cuddh_solver_result *out, double *h_res, double *h_time)
    {
        return guarded([&] { gmres_ddh(n, x, ddh, b, m, maxit, tol, verbose, max_seconds, GmresOptions{Orthogonalization::mgs, 0, Arithmetic::complex}, out, h_res, h_time); });
    }
    int cuddh_gmres_callback_cplx(int n, void *x, cuddh_action_cb cb, void *ctx, const void *b, int is_f64, int m, int maxit, double tol,
                                  int verbose, double max_seconds, cuddh_solver_result *out, double *h_res, double *h_time)
    {
        return guarded([&] { gmres_callback(n, x, cb, ctx, nullptr, b, is_f64, m, maxit, tol, verbose, max_seconds, GmresOptions{Orthogonalization::mgs, 0, Arithmetic::complex}, out, h_res, h_time); });
    }

    // ---- the small problem of a cycle on host arrays (csrc/src/gmres_small.hpp): no GPU
    int cuddh_gmres_small_problem(int is_complex, int is_f64, int m, int ncols, const void *h_cols, double beta, void *y_out, double *est_out)
    {
        return guarded([&]
        {
            if (!gmres_small_problem(is_complex, is_f64, m, ncols, h_cols, beta, y_out, est_out))
                throw std::runtime_error("gmres small problem: need m >= 1, 1 <= ncols <= m and non-null h_cols, y_out, est_out.");
        });
    }
}
