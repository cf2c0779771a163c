"""Python mirror of the reference's operator interface for the hot path.

Same names and argument meaning as the C++ classes of cuddh.hpp (Mesh2D, Basis,
H1Space, FaceSpace, EnsembleSpace, StiffnessMatrix, MassMatrix, FaceMassMatrix,
DDH, gmres); every method forwards to libcuddh_amd.so.  Device vectors are
torch CUDA tensors (torch is only the allocator / stream provider); host arrays
are numpy.  Column-major (Fortran) shapes throughout, as in the reference.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _native as N

lib = N.lib


def _ptr(t, dtype=None, numel=None, what="tensor"):
    """Device pointer of a torch tensor (None -> NULL).  dtype: "f64" / "f32" / a torch dtype the entry point reads or
    writes; numel: the least number of elements it touches.  A tensor of another type or a shorter one would otherwise become
    an out-of-bounds device access behind the C ABI instead of a Python error."""
    if t is None:
        return None
    if not t.is_cuda:
        raise ValueError(f"{what}: expected a CUDA tensor")
    if not t.is_contiguous():
        raise ValueError(f"{what}: expected a contiguous tensor")
    if dtype is not None:
        import torch

        want = {"f64": torch.float64, "f32": torch.float32, "i32": torch.int32}.get(dtype, dtype)
        if t.dtype != want:
            raise ValueError(f"{what}: expected dtype {want}, got {t.dtype}")
    if numel is not None and t.numel() < numel:
        raise ValueError(f"{what}: expected at least {numel} elements, got {t.numel()}")
    return C.c_void_p(t.data_ptr())


def _h(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def use_torch_stream() -> None:
    """Make the library launch on torch's current CUDA stream."""
    import torch

    lib.cuddh_set_stream(C.c_void_p(torch.cuda.current_stream().cuda_stream))


def device_count() -> int:
    return int(lib.cuddh_hip_device_count())


def quadrature(n: int, kind: str = "lobatto"):
    x = np.empty(n)
    w = np.empty(n)
    N.check_capi(lib.cuddh_quadrature(n, 0 if kind == "legendre" else 1, _h(x), _h(w)), "quadrature")
    return x, w


class Basis:
    def __init__(self, n: int):
        self.n = n
        self._h = N.handle(lib.cuddh_basis_create(n), "Basis")

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and lib is not None:  # `lib` may already be torn down at interpreter exit
            try:
                lib.cuddh_basis_destroy(h)
            except Exception:  # noqa: BLE001
                pass

    def size(self) -> int:
        return self.n

    def eval(self, x) -> np.ndarray:
        x = np.ascontiguousarray(x, dtype=np.float64)
        P = np.empty((len(x), self.n), order="F")
        N.check_capi(lib.cuddh_basis_eval(self._h, len(x), _h(x), _h(P)), "Basis.eval")
        return P

    def deriv(self, x) -> np.ndarray:
        x = np.ascontiguousarray(x, dtype=np.float64)
        D = np.empty((len(x), self.n), order="F")
        N.check_capi(lib.cuddh_basis_deriv(self._h, len(x), _h(x), _h(D)), "Basis.deriv")
        return D


class Mesh2D:
    def __init__(self, handle):
        self._h = handle

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and lib is not None:  # `lib` may already be torn down at interpreter exit
            try:
                lib.cuddh_mesh_destroy(h)
            except Exception:  # noqa: BLE001
                pass

    @staticmethod
    def uniform_rect(nx, ax, bx, ny, ay, by) -> "Mesh2D":
        return Mesh2D(N.handle(lib.cuddh_mesh_uniform_rect(nx, ax, bx, ny, ay, by), "Mesh2D.uniform_rect"))

    @staticmethod
    def from_vertices(xy: np.ndarray, elems: np.ndarray) -> "Mesh2D":
        """xy: (2, n_pts) F-order or (n_pts, 2) C-order; elems: (n_elem, 4) C-order vertex ids."""
        xy = np.ascontiguousarray(xy, dtype=np.float64)
        elems = np.ascontiguousarray(elems, dtype=np.int32)
        return Mesh2D(N.handle(lib.cuddh_mesh_from_vertices(xy.size // 2, _h(xy), elems.size // 4, _h(elems)), "Mesh2D.from_vertices"))

    @staticmethod
    def grid_cells(nx, ax, bx, ny, ay, by, present) -> "Mesh2D":
        """A grid mesh with missing cells: the cells of uniform_rect(nx, ax, bx, ny, ay, by) where present[j, i] is true
        (present: (ny, nx) bool, at least one true), in ascending cell index i + nx j with uniform_rect's corner order and
        vertex coordinates, the unused vertices dropped; built through from_vertices.  WaveHoltz(sweep="lattice") takes such a
        mesh (an obstacle, an L-shape, a staircase): csrc/kernels/wave_cells.hip, DESIGN 4.5.4."""
        present = np.asarray(present)
        if present.shape != (int(ny), int(nx)):
            raise ValueError(f"Mesh2D.grid_cells: present must have shape (ny, nx) = ({ny}, {nx}), not {present.shape}")
        flags = np.ascontiguousarray(present != 0, dtype=np.uint8)
        if not flags.any():
            raise ValueError("Mesh2D.grid_cells: at least one cell must be present")
        return Mesh2D(N.handle(lib.cuddh_mesh_grid_cells(int(nx), ax, bx, int(ny), ay, by, _h(flags)), "Mesh2D.grid_cells"))

    @staticmethod
    def load(directory) -> "Mesh2D":
        """the reference's text format: info.txt, coordinates.txt, elements.txt (tests/load_unstructured_square.cpp:11-55)"""
        return Mesh2D(N.handle(lib.cuddh_mesh_load(str(directory).encode()), "Mesh2D.load"))

    def refined(self, times: int = 1) -> "Mesh2D":
        """uniform refinement: every quadrilateral -> 4 (edge midpoints + centroid), `times` rounds"""
        return Mesh2D(N.handle(lib.cuddh_mesh_refined(self._h, int(times)), "Mesh2D.refined"))

    def partition(self, n_parts: int) -> np.ndarray:
        """element labels in [0, n_parts) for EnsembleSpace: compact, equally sized sets (centroid Morton order)"""
        out = np.empty(self.n_elem(), dtype=np.int32)
        N.check_capi(lib.cuddh_mesh_partition(self._h, int(n_parts), _h(out)), "Mesh2D.partition")
        return out

    def n_elem(self):
        return lib.cuddh_mesh_n_elem(self._h)

    def n_edges(self):
        return lib.cuddh_mesh_n_edges(self._h)

    def n_nodes(self):
        return lib.cuddh_mesh_n_nodes(self._h)

    def min_h(self):
        return lib.cuddh_mesh_min_h(self._h)

    def boundary_edges(self) -> np.ndarray:
        out = np.empty(lib.cuddh_mesh_n_boundary_edges(self._h), dtype=np.int32)
        N.check_capi(lib.cuddh_mesh_boundary_edges(self._h, _h(out)))
        return out

    def vertices(self) -> np.ndarray:
        """(n_nodes, 2) vertex coordinates"""
        out = np.empty((self.n_nodes(), 2))
        N.check_capi(lib.cuddh_mesh_vertices(self._h, _h(out)))
        return out

    def elements(self) -> np.ndarray:
        """(n_elem, 4) corner vertex ids, counter-clockwise"""
        out = np.empty((self.n_elem(), 4), dtype=np.int32)
        N.check_capi(lib.cuddh_mesh_elements(self._h, _h(out)))
        return out

    def edges(self) -> np.ndarray:
        """(n_edges, 8): type(1=boundary), node0, node1, elem0, elem1, side0, side1, delta"""
        out = np.empty((self.n_edges(), 8), dtype=np.int32)
        N.check_capi(lib.cuddh_mesh_edges(self._h, _h(out)))
        return out


class H1Space:
    def __init__(self, mesh: Mesh2D, basis: Basis):
        self.mesh, self.basis = mesh, basis
        self._h = N.handle(lib.cuddh_h1space_create(mesh._h, basis._h), "H1Space")

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and lib is not None:  # `lib` may already be torn down at interpreter exit
            try:
                lib.cuddh_h1space_destroy(h)
            except Exception:  # noqa: BLE001
                pass

    def size(self) -> int:
        return lib.cuddh_h1space_size(self._h)

    def global_indices(self) -> np.ndarray:
        nb = self.basis.n
        I = np.empty((nb, nb, self.mesh.n_elem()), dtype=np.int32, order="F")
        N.check_capi(lib.cuddh_h1space_global_indices(self._h, _h(I)))
        return I

    def physical_coordinates(self) -> np.ndarray:
        X = np.empty((2, self.size()), order="F")
        N.check_capi(lib.cuddh_h1space_coordinates(self._h, _h(X)))
        return X


class FaceSpace:
    def __init__(self, fem: H1Space, faces):
        self.fem = fem
        self.faces = np.ascontiguousarray(faces, dtype=np.int32)
        self._h = N.handle(lib.cuddh_facespace_create(fem._h, len(self.faces), _h(self.faces)), "FaceSpace")

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and lib is not None:  # `lib` may already be torn down at interpreter exit
            try:
                lib.cuddh_facespace_destroy(h)
            except Exception:  # noqa: BLE001
                pass

    def size(self):
        return lib.cuddh_facespace_size(self._h)

    def n_faces(self):
        return len(self.faces)

    def subspace_indices(self) -> np.ndarray:
        I = np.empty((self.fem.basis.n, len(self.faces)), dtype=np.int32, order="F")
        N.check_capi(lib.cuddh_facespace_subspace_indices(self._h, _h(I)))
        return I

    def global_indices(self) -> np.ndarray:
        p = np.empty(self.size(), dtype=np.int32)
        N.check_capi(lib.cuddh_facespace_global_indices(self._h, _h(p)))
        return p

    def restrict(self, x, y):
        N.check_capi(lib.cuddh_facespace_restrict(self._h, _ptr(x, "f64", self.fem.size(), "x"), _ptr(y, "f64", self.size(), "y")), "restrict")

    def prolong(self, x, y):
        N.check_capi(lib.cuddh_facespace_prolong(self._h, _ptr(x, "f64", self.size(), "x"), _ptr(y, "f64", self.fem.size(), "y")), "prolong")

    def orth(self, x):
        N.check_capi(lib.cuddh_facespace_orth(self._h, _ptr(x, "f64", self.fem.size(), "x")), "orth")


class EnsembleSpace:
    _SHAPES = {
        "gI": lambda d, nb: (d[3], d[0]),
        "sizes": lambda d, nb: (d[0],),
        "elements": lambda d, nb: (d[1], d[0]),
        "n_elems": lambda d, nb: (d[0],),
        "faces": lambda d, nb: (d[2], d[0]),
        "n_faces": lambda d, nb: (d[0],),
        "sI": lambda d, nb: (nb, nb, d[1], d[0]),
        "fI": lambda d, nb: (nb, d[2], d[0]),
        "pI": lambda d, nb: (d[4], d[0]),
        "fsizes": lambda d, nb: (d[0],),
        "cmap": lambda d, nb: (4, d[5]),
    }

    def __init__(self, fem: H1Space, n_spaces: int, labels):
        self.fem = fem
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        self._h = N.handle(lib.cuddh_ensemble_create(fem._h, n_spaces, _h(labels)), "EnsembleSpace")
        d = np.empty(6, dtype=np.int32)
        N.check_capi(lib.cuddh_ensemble_dims(self._h, _h(d)))
        self.dims = d

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and lib is not None:  # `lib` may already be torn down at interpreter exit
            try:
                lib.cuddh_ensemble_destroy(h)
            except Exception:  # noqa: BLE001
                pass

    def array(self, name: str) -> np.ndarray:
        shape = self._SHAPES[name](self.dims, self.fem.basis.n)
        out = np.empty(shape, dtype=np.int32, order="F")
        if out.size:
            N.check_capi(lib.cuddh_ensemble_array(self._h, name.encode(), _h(out)))
        return out


class _Operator:
    """y = A x (`action(x, y)`) and y += c A x (`action(c, x, y)`) on device vectors."""

    def __init__(self, handle, keepalive=(), n=None):
        self._h = handle
        self._keep = keepalive
        self._n = n  # length of the vectors action() reads and writes (None: not checked)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and lib is not None:  # `lib` may already be torn down at interpreter exit
            try:
                lib.cuddh_operator_destroy(h)
            except Exception:  # noqa: BLE001
                pass

    def kernel(self) -> str:
        """kernel instantiation action() launches, e.g. 'helm_lane_kernel<4,5,8,NT=1,UG=0> pe=64' (single operators build
        their plan on the first action(): 'generic' before that and when no specialised kernel exists)"""
        buf = C.create_string_buffer(160)
        N.check_capi(lib.cuddh_operator_kernel_name(self._h, buf, 160), "kernel")
        return buf.value.decode()

    def action(self, *args):
        if len(args) == 2:
            x, y = args
            N.check_capi(lib.cuddh_operator_apply(self._h, _ptr(x, "f64", self._n, "x"), _ptr(y, "f64", self._n, "y")), "action")
        else:
            c, x, y = args
            N.check_capi(lib.cuddh_operator_apply_add(self._h, float(c), _ptr(x, "f64", self._n, "x"), _ptr(y, "f64", self._n, "y")), "action")


class StiffnessMatrix(_Operator):
    def __init__(self, fem: H1Space, nq: int = 0):
        super().__init__(N.handle(lib.cuddh_stiffness_create(fem._h, nq), "StiffnessMatrix"), (fem,), fem.size())


class MassMatrix(_Operator):
    def __init__(self, fem: H1Space, a=None):
        super().__init__(N.handle(lib.cuddh_mass_create(fem._h, _ptr(a, "f64", fem.size(), "a")), "MassMatrix"), (fem, a), fem.size())


class DiagInvMassMatrix(_Operator):
    def __init__(self, fem: H1Space, a=None):
        super().__init__(N.handle(lib.cuddh_diaginv_mass_create(fem._h, _ptr(a, "f64", fem.size(), "a")), "DiagInvMassMatrix"), (fem, a), fem.size())


class FaceMassMatrix(_Operator):
    def __init__(self, fs: FaceSpace, a=None):
        super().__init__(N.handle(lib.cuddh_facemass_create(fs._h, _ptr(a, "f64", fs.size(), "a")), "FaceMassMatrix"), (fs, a), fs.size())


class DiagInvFaceMassMatrix(_Operator):
    def __init__(self, fs: FaceSpace, a=None):
        super().__init__(N.handle(lib.cuddh_diaginv_facemass_create(fs._h, _ptr(a, "f64", fs.size(), "a")), "DiagInvFaceMassMatrix"), (fs, a), fs.size())


class HelmholtzOperator(_Operator):
    """Fused [u;v] -> [Au;Av] of reference examples/Helmholtz.hpp:28-56."""

    def __init__(self, omega: float, a2x, ax, fem: H1Space, fs: FaceSpace):
        super().__init__(N.handle(lib.cuddh_helmholtz_create(float(omega), _ptr(a2x, "f64", fem.size(), "a2x"), _ptr(ax, "f64", fs.size(), "ax"), fem._h, fs._h),
                                  "HelmholtzOperator"), (fem, fs, a2x, ax), 2 * fem.size())

    def action_unfused(self, x, y):
        N.check_capi(lib.cuddh_helmholtz_apply_unfused(self._h, _ptr(x, "f64", self._n, "x"), _ptr(y, "f64", self._n, "y")), "action_unfused")

    def fused(self) -> bool:
        return bool(lib.cuddh_helmholtz_is_fused(self._h))

    def bytes_per_apply(self, actual: bool = False) -> int:
        return int(lib.cuddh_helmholtz_bytes(self._h, 1 if actual else 0))

    # ---- plan-native vector ordering (cuddh_hip.h: cuddh_hip_helmholtz_apply_native)
    def has_native(self) -> bool:
        return bool(lib.cuddh_helmholtz_has_native(self._h))

    def to_native(self, x, z):
        N.check_capi(lib.cuddh_helmholtz_to_native(self._h, _ptr(x, "f64", self._n, "x"), _ptr(z, "f64", self._n, "z")), "HelmholtzOperator.to_native")

    def from_native(self, z, y):
        N.check_capi(lib.cuddh_helmholtz_from_native(self._h, _ptr(z, "f64", self._n, "z"), _ptr(y, "f64", self._n, "y")), "HelmholtzOperator.from_native")

    def action_native(self, z_in, z_out):
        N.check_capi(lib.cuddh_helmholtz_apply_native(self._h, _ptr(z_in, "f64", self._n, "z_in"), _ptr(z_out, "f64", self._n, "z_out")), "HelmholtzOperator.action_native")

    def gmres(self, x, b, m: int, maxit: int, tol: float = 1e-6, verbose: int = 0, max_seconds: float = 6 * 60 * 60, orth: str = "mgs",
              augment: int = 0) -> "SolverOut":
        """HelmholtzOperator::gmres: x, b in the reference ordering; iteration vectors in plan-native ordering when the plan has one.
        orth: "mgs" or "cgs2"; augment: 0 or the number of corrections an LGMRES cycle is augmented with (see gmres)"""
        code = _orth_code(orth)
        aug = _augment_count(augment, m)
        aug_arg = (aug,) if aug else ()  # augment = 0 leaves the argument out: the call _gmres_entry has always had, which tests replace
        res = N.SolverResult()
        h_res = np.zeros(maxit + 2)
        h_time = np.zeros(maxit + 2)
        N.check_capi(_gmres_entry("cuddh_gmres_helmholtz", code, (self._h, _ptr(x, "f64", self._n, "x"), _ptr(b, "f64", self._n, "b"), m, maxit, float(tol), verbose,
                                                                   float(max_seconds)), res, h_res, h_time, *aug_arg), "HelmholtzOperator.gmres")
        return _solver_out(res, h_res, h_time)

    def bytes_native(self) -> int:
        return int(lib.cuddh_helmholtz_bytes(self._h, 3))

    def bytes_affine(self) -> int:
        """SURVEY 8d's "affine" figure when the plan reads the stiffness metric from one uniform table (0 otherwise)"""
        return int(lib.cuddh_helmholtz_bytes(self._h, 2))


# integrand ids of cuddh_capi.h
GAUSSIANS, ALPHA_DISK, MASS_POLY, STIFF_NEG_LAPLACIAN, STIFF_FUNC, CONSTANT, ALPHA_DISK_SQ = range(7)


def linear_functional(fem: H1Space, integrand: int, F, param: float = 0.0, nq: int = 0, c: float = 1.0, accumulate: bool = False):
    N.check_capi(lib.cuddh_linear_functional(fem._h, nq, integrand, float(param), float(c), int(accumulate), _ptr(F)), "LinearFunctional")


def face_linear_functional(fs: FaceSpace, integrand: int, F, param: float = 0.0, nq: int = 0, c: float = 1.0, accumulate: bool = False):
    N.check_capi(lib.cuddh_face_linear_functional(fs._h, nq, integrand, float(param), float(c), int(accumulate), _ptr(F)), "FaceLinearFunctional")


def nodal_values(fem: H1Space, integrand: int, out, param: float = 0.0):
    N.check_capi(lib.cuddh_nodal_values(fem._h, integrand, float(param), _ptr(out)), "nodal_values")


@dataclass
class SolverOut:
    success: bool
    num_iter: int
    num_matvec: int
    res_norm: list = field(default_factory=list)
    time: list = field(default_factory=list)


def _solver_out(res: N.SolverResult, h_res, h_time) -> SolverOut:
    n = res.n_res
    return SolverOut(bool(res.success), res.num_iter, res.num_matvec, list(h_res[:n]), list(h_time[:n]))


class DDH:
    """Substructured Helmholtz solver (reference include/DDH.hpp).  precision 'f32' is the
    reference's; 'f64' is the parity mode with double traces.

    kernel selects the local-solve kernel (cuddh_hip_ddh_plan_create): 0 auto, 1 generic, 2 wavefront per subdomain,
    3 / 4 / 5 / 7 fp32 forms (5: dense element matrix on the matrix cores), 6 n_basis 8, 8 = kernel 5 in fp64
    (precision='f64', n_basis 4, uniform metric; never picked by auto).  Requested where it does not apply, 5 to 8 raise on
    first use.  DDH.from_labels builds the solver on any mesh from element labels (kernels 9 and 10).

    block: elements per subdomain side.  None, 0 or 16 / n_basis is the reference's size; any block >= 1 with
    n_basis^2 block^2 <= 1024 that divides nx and ny is accepted, anything else raises here.  Off the reference's size the
    kernels are 1 (any block), 11 (n_basis 4, block 8, 'f32': one 8x8 block per wavefront; what auto picks there) and 12
    (n_basis 5, block 4, 'f32', rectangles: one element per lane, four 4x4 blocks per wavefront; time_step "mesh" and "rk2"
    only; what auto picks there from the subdomain count at which it measured faster than kernel 1) and 13 (on request only:
    the local solves of kernel 5's element-lane form at n_basis 4 and of kernel 12 at n_basis 5, block 4, 'f32', four
    subdomains per wavefront, on any time_step; "rk2" only; sweep_form() is 0 and set_sweep_form(2) raises).  Larger
    subdomains need fewer GMRES iterations and shorter Krylov vectors but more WaveHoltz iterations (set_wh_iters) for the
    same accuracy.  info()["nel1d"] reports the block in effect.

    time_step: where the local solves take their time step from.  "mesh" (the default, the reference's): one grid from the
    mesh width alone, dt = 0.1 h / n_basis^2, whatever the coefficient; where a < 1 (wave speed 1 / a > 1) the explicit
    stepping then runs past its usable range and the local solves blow up.  "coefficient": subdomain s marches
    r_s times as many steps per period, r_s = max(1, ceil(1 / min a over its dofs)); a == 1 everywhere is "mesh" bit for bit.
    An integer array (one ratio >= 1 per subdomain): those ratios.  time_ratios() returns r; info()["nt"], info()["dt"] and
    table("filter" | "cs" | "sn") stay the base grid's, table("filter@5") etc. are those of the grid of 5 x the mesh grid's steps.
    A bad array, a non-finite or non-positive a under "coefficient", and a ratio above 256 raise ValueError here.
    Kernels that hold one subdomain per wavefront or workgroup take any time_step; of those that hold several, kernel 13
    alone does (kernel=5 then runs its matrix form, auto leaves 6, 7 and 12 for 1, and 6, 7 and 12 on request raise on first
    use).  A wavefront of kernel 13 marches once per distinct ratio among its four subdomains and costs the sum of those
    marches.  action(), rhs() and local_traces over all subdomains run them sorted by ratio, so at most (number of distinct
    ratios - 1) wavefronts hold more than one; sub-ranges and local_traces_listed run in the caller's order: list
    subdomains of one ratio next to each other, in groups of four, or a wavefront pays for every ratio it holds.

    integrator, coarsen: how the local solves step in time.  "rk2" (the default, the reference's): the explicit midpoint rule on
    the mesh grid, two stiffness sweeps per step; coarsen must be None or 1.  "rk4": classical Runge-Kutta, four sweeps per
    step, on the base grid of nt = ceil(nt_mesh / coarsen) steps of dt = T / nt, nt_mesh the mesh grid's count; coarsen is an
    integer in [1, 16], None means 4.  time_step composes unchanged: subdomain s marches r_s nt steps.  info()["nt"],
    info()["dt"], table("filter" | "cs" | "sn") and table("filter@r") are those of the coarsened base grid; integrator()
    returns ("rk4", 4).  The mesh grid is as fine as it is for the midpoint rule's stability, not for accuracy: RK4 at coarsen 4
    is closer to the exact local solve than RK2 on the mesh grid, in half the sweeps.  Stable range: with
    a == 1 it ends near coarsen 23 (hence the cap of 16); it scales with min a over a subdomain unless
    time_step="coefficient" compensates: with a = 0.2 under "mesh", coarsen <= 4.  Kernels 1, 2, 5 (matrix form) and 8 (and
    from_labels' 9 and 10) have an RK4 form; auto picks among them (info()["kernel"]), any other kernel on request (3, 4, 6, 7, 11, 12, 13) raises RuntimeError on first use.  A bad
    name, a coarsen that is no integer in [1, 16] and coarsen > 1 with "rk2" raise ValueError here."""

    _INT_TABLES = ("B", "gI", "sI")

    def __init__(self, omega: float, h_a: np.ndarray, fem: H1Space, nx: int, ny: int, precision: str = "f32", kernel: int = 0,
                 block: int | None = None, time_step="mesh", integrator: str = "rk2", coarsen: int | None = None):
        self.fem = fem
        self.f64 = precision == "f64"
        scheme, coarsen = self._integrator(integrator, coarsen)
        h_a = np.ascontiguousarray(h_a, dtype=np.float64)
        if scheme == 1:
            policy, ratios = self._time_step_policy(time_step)
            h = lib.cuddh_ddh_create_integrator(float(omega), _h(h_a), fem._h, nx, ny, int(block or 0), int(self.f64), kernel, policy,
                                                None if ratios is None else _h(ratios), 0 if ratios is None else int(ratios.size),
                                                scheme, coarsen)
            if not h and N.last_error().startswith(("DDH error: time step", "DDH error: integrator")):
                raise ValueError(f"DDH: {N.last_error()}")
            self._h = N.handle(h, "DDH")
        elif isinstance(time_step, str) and time_step == "mesh":
            if block is None:
                self._h = N.handle(lib.cuddh_ddh_create(float(omega), _h(h_a), fem._h, nx, ny, int(self.f64), kernel), "DDH")
            else:
                self._h = N.handle(lib.cuddh_ddh_create_block(float(omega), _h(h_a), fem._h, nx, ny, int(block), int(self.f64), kernel), "DDH")
        else:
            policy, ratios = self._time_step_policy(time_step)
            h = lib.cuddh_ddh_create_timegrid(float(omega), _h(h_a), fem._h, nx, ny, int(block or 0), int(self.f64), kernel, policy,
                                              None if ratios is None else _h(ratios), 0 if ratios is None else int(ratios.size))
            if not h and N.last_error().startswith("DDH error: time step"):
                raise ValueError(f"DDH: {N.last_error()}")
            self._h = N.handle(h, "DDH")
        self.omega = float(omega)

    @staticmethod
    def _integrator(integrator, coarsen):
        """(scheme, coarsen) of cuddh_ddh_create_integrator, or ValueError; "rk2" is (0, 1): the creators without an integrator"""
        if not isinstance(integrator, str) or integrator not in ("rk2", "rk4"):
            raise ValueError(f"DDH: integrator must be 'rk2' or 'rk4', not {integrator!r}")
        if coarsen is None:
            coarsen = 1 if integrator == "rk2" else 4
        if isinstance(coarsen, (bool, np.bool_)) or not isinstance(coarsen, (int, np.integer)):
            raise ValueError(f"DDH: coarsen must be an integer in [1, 16], not {coarsen!r}")
        if not 1 <= coarsen <= 16:
            raise ValueError(f"DDH: coarsen must lie in [1, 16], got {int(coarsen)}")
        if integrator == "rk2" and coarsen != 1:
            raise ValueError("DDH: integrator 'rk2' marches on the mesh grid (coarsen 1) only; a coarser grid needs 'rk4'")
        return (0 if integrator == "rk2" else 1), int(coarsen)

    @staticmethod
    def _time_step_policy(time_step):
        """(policy, ratios) of cuddh_ddh_create_timegrid; what is wrong with an array is refused here"""
        if isinstance(time_step, str):
            if time_step not in ("mesh", "coefficient"):
                raise ValueError(f"DDH: time_step must be 'mesh', 'coefficient' or an integer array, not {time_step!r}")
            return (0 if time_step == "mesh" else 1), None
        ratios = np.asarray(time_step)
        if ratios.ndim != 1 or not np.issubdtype(ratios.dtype, np.integer):
            raise ValueError("DDH: time_step ratios must be a one-dimensional integer array, one entry per subdomain")
        if ratios.size and (ratios.min() < 1 or ratios.max() > 256):
            raise ValueError(f"DDH: time_step ratios must lie in [1, 256], got {int(ratios.min())} .. {int(ratios.max())}")
        return 2, np.ascontiguousarray(ratios, dtype=np.int32)

    @classmethod
    def from_labels(cls, omega: float, h_a: np.ndarray, fem: H1Space, labels, precision: str = "f32", kernel: int = 0,
                    time_step="mesh", integrator: str = "rk2", coarsen: int | None = None, time_ratios=None) -> "DDH":
        """DDH on any mesh with subdomain s = the elements labelled s (one label per element, e.g. Mesh2D.partition), labels in
        [0, n_domains) with n_domains = max(labels) + 1; every subdomain non-empty with at most 256 element nodes.
        kernel: 0 auto, 9 one wavefront per subdomain (n_basis 4, <= 16 elements per subdomain), 10 one workgroup per
        subdomain.  info()["nel1d"] is 0.  Invalid labels or kernels raise here, before anything runs on the device.
        integrator, coarsen: as in DDH(...), with the same ValueErrors; kernels 9 and 10 both have an RK4 form, so auto picks
        as it does for RK2.
        time_ratios: the per-subdomain time grids of DDH(..., time_step=).  None: every subdomain on the base grid;
        "coefficient": r_s = max(1, ceil((1 - 1e-9) / min a over the subdomain's dofs)); or a one-dimensional integer array,
        one ratio in [1, 256] per label.  A bad array, the wrong length, another name and a non-finite or non-positive a under
        "coefficient" raise ValueError.  time_ratios(), integrator(), info() and table("filter@r") work as on block plans.
        time_step accepts "mesh" alone and raises ValueError for anything else, as it always has here, which is why the
        per-subdomain policy has a keyword of its own."""
        if not (isinstance(time_step, str) and time_step == "mesh"):
            raise ValueError("DDH.from_labels: time_step is 'mesh' only; per-subdomain time grids are time_ratios='coefficient' or an integer array")
        scheme, coarsen = cls._integrator(integrator, coarsen)
        if time_ratios is None:
            policy, ratios = 0, None
        elif isinstance(time_ratios, str):
            if time_ratios != "coefficient":
                raise ValueError(f"DDH.from_labels: time_ratios must be None, 'coefficient' or an integer array, not {time_ratios!r}")
            policy, ratios = 1, None
        else:
            policy, ratios = cls._time_step_policy(time_ratios)
        labels = np.ascontiguousarray(labels)
        n_elem = fem.mesh.n_elem()
        if labels.ndim != 1 or labels.size != n_elem:
            raise ValueError(f"DDH.from_labels: {labels.size} labels for {n_elem} elements")
        if not np.issubdtype(labels.dtype, np.integer):
            raise ValueError("DDH.from_labels: labels must be integers")
        if labels.size and (labels.min() < 0 or labels.max() >= 2**31 - 1):
            raise ValueError(f"DDH.from_labels: label {int(labels.min()) if labels.min() < 0 else int(labels.max())} out of range")
        n_domains = int(labels.max()) + 1 if labels.size else 0
        labels = labels.astype(np.int32)
        self = cls.__new__(cls)
        self.fem = fem
        self.f64 = precision == "f64"
        h_a = np.ascontiguousarray(h_a, dtype=np.float64)
        if scheme == 0 and policy == 0:
            self._h = N.handle(lib.cuddh_ddh_create_labels(float(omega), _h(h_a), fem._h, n_domains, _h(labels), int(self.f64), int(kernel)),
                               "DDH.from_labels")
        else:
            if ratios is not None and ratios.size != n_domains:
                raise ValueError(f"DDH.from_labels: {ratios.size} time_ratios for {n_domains} subdomains")
            h = lib.cuddh_ddh_create_labels_integrator(float(omega), _h(h_a), fem._h, n_domains, _h(labels), int(self.f64), int(kernel), policy,
                                                       None if ratios is None else _h(ratios), 0 if ratios is None else int(ratios.size),
                                                       scheme, coarsen)
            if not h and N.last_error().startswith(("DDH error: time step", "DDH error: integrator")):
                raise ValueError(f"DDH.from_labels: {N.last_error()}")
            self._h = N.handle(h, "DDH.from_labels")
        self.omega = float(omega)
        return self

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and lib is not None:  # `lib` may already be torn down at interpreter exit
            try:
                lib.cuddh_ddh_destroy(h)
            except Exception:  # noqa: BLE001
                pass

    def size(self) -> int:
        return lib.cuddh_ddh_size(self._h)

    @property
    def trace_dtype(self):
        import torch

        return torch.float64 if self.f64 else torch.float32

    def info(self) -> dict:
        info = np.zeros(8, dtype=np.int32)
        dt = C.c_double()
        N.check_capi(lib.cuddh_ddh_info(self._h, _h(info), C.byref(dt)), "DDH.info")
        keys = ("n_domains", "nt", "n_lambda", "mx_dof", "mx_fdof", "nel1d", "kernel", "is_f64")
        out = dict(zip(keys, map(int, info)))
        out["dt"] = dt.value
        return out

    def time_ratios(self) -> np.ndarray:
        """per subdomain: how many times the mesh grid's steps its local solve marches per period (time_step)"""
        n = lib.cuddh_ddh_time_ratios(self._h, None)
        if n < 0:
            raise RuntimeError(f"DDH.time_ratios failed: {N.last_error()}")
        out = np.zeros(n, dtype=np.int32)
        lib.cuddh_ddh_time_ratios(self._h, _h(out))
        return out

    def integrator(self) -> tuple:
        """(name, coarsen) of the local solves' time stepping: ("rk2", 1) unless built with the integrator argument"""
        scheme, coarsen = C.c_int(), C.c_int()
        N.check_capi(lib.cuddh_ddh_integrator(self._h, C.byref(scheme), C.byref(coarsen)), "DDH.integrator")
        return ("rk4" if scheme.value == 1 else "rk2"), coarsen.value

    def set_wh_iters(self, n: int = 5):
        """Verification knob: WaveHoltz iterations per local solve (reference: 5, source/DDH.cpp:136)."""
        N.check_capi(lib.cuddh_ddh_set_wh_iters(self._h, int(n)), "DDH.set_wh_iters")

    def set_sweep_form(self, form: int = 0):
        """Kernel 5's sweep, for every launch of this plan: 0 auto, 1 matrix form, 2 element-lane form, 3 the same with the
        other copy of every shared node publishing (a check: same results).  2 and 3 are refused where the plan cannot take them
        (cuddh_hip_ddh_plan_set_sweep_form)."""
        N.check_capi(lib.cuddh_ddh_set_sweep_form(self._h, int(form)), "DDH.set_sweep_form")

    def sweep_form(self) -> int:
        """The form in effect: 1 matrix, 2 element-lane (3 if requested); 0 when the plan is not kernel 5."""
        form = lib.cuddh_ddh_sweep_form(self._h)
        if form < 0:
            N.check_capi(form, "DDH.sweep_form")
        return form

    def set_chain_order(self, order: int = 0):
        """The summation order of the element-lane form's in-lane products, for every launch of this plan: 0 auto (paired where auto
        chose the form, pinned where set_sweep_form forced it), 1 pinned (the node-by-node loop's chains, bit for bit), 2 paired
        (7 packed instructions per register pair; the last bits differ).  2 is refused where the plan cannot take it
        (cuddh_hip_ddh_plan_set_chain_order)."""
        N.check_capi(lib.cuddh_ddh_set_chain_order(self._h, int(order)), "DDH.set_chain_order")

    def chain_order(self) -> int:
        """The order in effect: 1 pinned, 2 paired; 0 where the element-lane form is not in effect."""
        order = lib.cuddh_ddh_chain_order(self._h)
        if order < 0:
            N.check_capi(order, "DDH.chain_order")
        return order

    def set_forcing(self, forcing: int = 0):
        """Where the element-lane form's march applies the trace sources, for every launch of this plan: 0 auto (2 where form and
        order are auto too and auto gave the paired chains, else 1), 1 in every WaveHoltz pass, 2 in the first pass only (the later
        passes run a time loop without source terms and add the first pass's result; the last bits differ).  2 is refused where
        chain order 2 is (cuddh_hip_ddh_plan_set_forcing)."""
        N.check_capi(lib.cuddh_ddh_set_forcing(self._h, int(forcing)), "DDH.set_forcing")

    def forcing(self) -> int:
        """The forcing in effect: 1 every pass, 2 the first pass only; 0 where the paired chains are not in effect."""
        forcing = lib.cuddh_ddh_forcing(self._h)
        if forcing < 0:
            N.check_capi(forcing, "DDH.forcing")
        return forcing

    def set_march(self, march: int = 0):
        """How the march of forcing 2 carries the velocity, for every launch of this plan: 0 auto (2 where form, order and forcing
        are auto too and auto gave forcing 2, else 1), 1 as it is, 2 scaled, with the midpoint update folded into the sweep (fewer
        instructions per step; the last bits differ).  2 is refused where forcing 2 is (cuddh_hip_ddh_plan_set_march)."""
        N.check_capi(lib.cuddh_ddh_set_march(self._h, int(march)), "DDH.set_march")

    def march(self) -> int:
        """The march in effect: 1 or 2; 0 where forcing 2 is not in effect."""
        march = lib.cuddh_ddh_march(self._h)
        if march < 0:
            N.check_capi(march, "DDH.march")
        return march

    def set_head(self, head: int = 0):
        """What march 2 carries as the velocity, for every launch of this plan: 0 auto (2 wherever march 2 is in effect), 1
        q / (2 hm), 2 that times the head coefficient of the first sweep's chain, so that the chain opens on the state (one
        instruction per pair and step less; the last bits differ).  2 is refused where march 2 is (cuddh_hip_ddh_plan_set_head)."""
        N.check_capi(lib.cuddh_ddh_set_head(self._h, int(head)), "DDH.set_head")

    def head(self) -> int:
        """The head in effect: 1 or 2; 0 where march 2 is not in effect."""
        head = lib.cuddh_ddh_head(self._h)
        if head < 0:
            N.check_capi(head, "DDH.head")
        return head

    def set_assembly(self, assembly: int = 0):
        """How head 2 forms the neighbour sums of its sweeps, for every launch of this plan: 0 auto, 1 DPP on the vector pipe, 2
        every copy of a shared node fetches the other copy's partial sum over the LDS pipe and adds it itself (bit for bit the same
        results).  2 is refused where head 2 is not in effect (cuddh_hip_ddh_plan_set_assembly)."""
        N.check_capi(lib.cuddh_ddh_set_assembly(self._h, int(assembly)), "DDH.set_assembly")

    def assembly(self) -> int:
        """The assembly in effect: 1 or 2; 0 where head 2 is not in effect."""
        assembly = lib.cuddh_ddh_assembly(self._h)
        if assembly < 0:
            N.check_capi(assembly, "DDH.assembly")
        return assembly

    def set_owner_rule(self, last: bool):
        """Kernels 11, 12 and 13: the last copy of every node that elements share publishes instead of the first (a check: same results).
        Refused on any other kernel (cuddh_hip_ddh_plan_set_owner_rule)."""
        N.check_capi(lib.cuddh_ddh_set_owner_rule(self._h, 1 if last else 0), "DDH.set_owner_rule")

    def set_wave_priority(self, high: bool):
        """The local solves launched next take issue priority over other resident wavefronts (s_setprio); results unchanged."""
        N.check_capi(lib.cuddh_ddh_set_wave_priority(self._h, 1 if high else 0), "DDH.set_wave_priority")

    def table(self, name: str) -> np.ndarray:
        n = lib.cuddh_ddh_table(self._h, name.encode(), None, 1)
        if n < 0:
            raise RuntimeError(N.last_error())
        dtype = np.int32 if name in self._INT_TABLES else (np.float64 if self.f64 else np.float32)
        out = np.empty(int(n), dtype=dtype)
        if n:
            lib.cuddh_ddh_table(self._h, name.encode(), _h(out), 0)
        return out

    def rhs(self, f, b):
        N.check_capi(lib.cuddh_ddh_rhs(self._h, _ptr(f, "f64", 2 * self.fem.size(), "f"), _ptr(b, self.trace_dtype, self.size(), "b")), "DDH.rhs")

    def postprocess(self, lam, f, u):
        N.check_capi(lib.cuddh_ddh_postprocess(self._h, _ptr(lam, self.trace_dtype, self.size(), "lambda"), _ptr(f, "f64", 2 * self.fem.size(), "f"),
                                               _ptr(u, "f64", 2 * self.fem.size(), "u")), "DDH.postprocess")

    def action(self, x, y):
        N.check_capi(lib.cuddh_ddh_action(self._h, _ptr(x, self.trace_dtype, self.size(), "x"), _ptr(y, self.trace_dtype, self.size(), "y")), "DDH.action")

    def local_traces(self, d0, d1, f, lam, update):
        N.check_capi(lib.cuddh_ddh_local_traces(self._h, d0, d1, _ptr(f, "f64", 2 * self.fem.size(), "f"), _ptr(lam, self.trace_dtype, self.size(), "lambda"),
                                                 _ptr(update, self.trace_dtype, self.size(), "update")), "DDH.local_traces")

    def local_traces_listed(self, domains, f, lam, update):
        """local_traces for the subdomains listed in `domains` (int32 device tensor, distinct ids), one launch"""
        N.check_capi(lib.cuddh_ddh_local_traces_listed(self._h, _ptr(domains, "i32", domains.numel(), "domains"), int(domains.numel()),
                                                        _ptr(f, "f64", 2 * self.fem.size(), "f"), _ptr(lam, self.trace_dtype, self.size(), "lambda"),
                                                        _ptr(update, self.trace_dtype, self.size(), "update")), "DDH.local_traces_listed")

    def local_solution_listed(self, domains, lam, f, u, zero_u=True):
        """local_solution for the subdomains listed in `domains` (int32 device tensor, distinct ids), one launch"""
        N.check_capi(lib.cuddh_ddh_local_solution_listed(self._h, _ptr(domains, "i32", domains.numel(), "domains"), int(domains.numel()),
                                                          _ptr(lam, self.trace_dtype, self.size(), "lambda"), _ptr(f, "f64", 2 * self.fem.size(), "f"),
                                                          _ptr(u, "f64", 2 * self.fem.size(), "u"), int(zero_u)), "DDH.local_solution_listed")

    def local_solution(self, d0, d1, lam, f, u, zero_u=True):
        N.check_capi(lib.cuddh_ddh_local_solution(self._h, d0, d1, _ptr(lam, self.trace_dtype, self.size(), "lambda"), _ptr(f, "f64", 2 * self.fem.size(), "f"),
                                                   _ptr(u, "f64", 2 * self.fem.size(), "u"), int(zero_u)), "DDH.local_solution")


ORTHOGONALIZATIONS = {"mgs": 0, "cgs2": 1}


class WaveHoltz(_Operator):
    """Whole-domain WaveHoltz (csrc/include/cuddh/waveholtz.hpp): the filtered time-domain iteration for
    (K - w^2 M + i w H) U = f on the whole space, M = diag(a^2 m) and H = diag(a h) lumped, K the global StiffnessMatrix.
    An operator of size 2 ndof on z = [u; v] whose action is y = x - S x, so that
        W.rhs(f, b); gmres(W.size(), z, W, b, m, maxit, tol); W.solution(z, u)        (or W.solve(f, u, ...))
    solves it; U = u + i v / w.  It is not a check of DDH's fixed point, which is another discrete problem.

    h_a: HOST nodal coefficient (finite, positive).  integrator "rk2" (the mesh grid) or "rk4" on ceil(nt_mesh / coarsen) steps
    (coarsen in [1, 16], default 4), DDH's rules.  time_ratio: an integer in [1, 256] that multiplies the step count, or
    "coefficient" = max(1, ceil((1 - 1e-9) / min a)).  stiffness "gauss" (StiffnessMatrix(fem)) or "lobatto" (the collocated
    stiffness of the DDH local solves).  faces: edge ids of the absorbing faces, None = every boundary edge.
    sweep "operator" (the default: a stiffness apply and a stage kernel per sweep) or "lattice": one launch per sweep does the
    stiffness stencil and the stage on lattice-ordered vectors (csrc/kernels/wave_lattice.hip).  "lattice" needs stiffness
    "lobatto" and a uniform rectangle mesh, which is detected; every method takes and returns vectors in the space's order.
    A grid mesh with missing cells (Mesh2D.grid_cells: an obstacle, an L-shape, a staircase) is detected too, where the mesh is
    no full rectangle, and runs the same march on csrc/kernels/wave_cells.hip / wave_cells_f32.hip (info()["stiffness_kernel"]
    "wave_cells nb<n>"); faces=None makes the walls of a hole absorbing, faces= the outer edges only makes them sound-hard.
    launch "pair" is refused on such a mesh (ValueError, "launch").
    precision "f64" (the default) or "f32" (sweep "lattice" only): the lattice vectors are stored and the sweeps computed in fp32
    (csrc/kernels/wave_lattice_f32.hip), half the march's memory and bytes per sweep.  z, f, b and the solution stay float64; y =
    x - S x is formed in float64.  It is meant for tolerances around 1e-4: the fp32 operator's own defect is about 1e-6 relative,
    so a solve to 1e-6 or below wants "f64".
    launch "sweep" (the default: one launch per sweep) or "pair" (sweep "lattice" only, either precision): two sweeps per launch
    (csrc/kernels/wave_pair.hip, wave_pair_f32.hip): rk2_a with rk2_b, rk4_1 with rk4_2, rk4_3 with rk4_4.  The march is the
    per-sweep one bit for bit, in half the launches and about half the bytes.  Nothing selects "pair" by itself.
    cell_stiffness None (the default: exactly the calls above) or an array of fem.mesh.n_elem() finite positive floats, one beta
    per element in element order (sweep "lattice" only, launch "sweep" only, either precision, full and holed grids): the problem
    becomes -div(beta grad U) - w^2 a^2 U = f with beta constant on each element, on csrc/kernels/wave_weights.hip /
    wave_weights_f32.hip (info()["stiffness_kernel"] "wave_weights nb<n>").  time_ratio "coefficient" then is
    max(1, ceil((1 - 1e-9) max_e sqrt(beta_e) / min_{g in e} a_g)).  M and H keep their form, so the absorbing faces discretise
    beta dU/dn + i w a U = 0: the first-order absorbing condition only where beta = 1 along them.  A wrong length or dimension,
    a value that is not finite and positive, another sweep or launch "pair" raise ValueError before any native call.
    A bad name, a coarsen outside its range, coarsen > 1 with "rk2", a bad ratio, "lattice" with "gauss" and "f32" or "pair" without "lattice"
    raise ValueError before any native call; a mesh the lattice form cannot take raises ValueError with the native message."""

    STIFFNESS = ("gauss", "lobatto")
    SWEEPS = ("operator", "lattice")
    PRECISIONS = ("f64", "f32")
    LAUNCHES = ("sweep", "pair")

    def __init__(self, omega: float, h_a: np.ndarray, fem: H1Space, integrator: str = "rk2", coarsen: int | None = None, time_ratio=1,
                 stiffness: str = "gauss", faces=None, sweep: str = "operator", precision: str = "f64", launch: str = "sweep",
                 cell_stiffness=None):
        scheme, coarsen = self._integrator(integrator, coarsen)
        ratio = self._ratio(time_ratio)
        if not isinstance(stiffness, str) or stiffness not in self.STIFFNESS:
            raise ValueError(f"WaveHoltz: stiffness must be 'gauss' or 'lobatto', not {stiffness!r}")
        if not isinstance(sweep, str) or sweep not in self.SWEEPS:
            raise ValueError(f"WaveHoltz: sweep must be 'operator' or 'lattice', not {sweep!r}")
        if sweep == "lattice" and stiffness != "lobatto":
            raise ValueError("WaveHoltz: sweep 'lattice' is the collocated stiffness; it needs stiffness 'lobatto'")
        if not isinstance(precision, str) or precision not in self.PRECISIONS:
            raise ValueError(f"WaveHoltz: precision must be 'f64' or 'f32', not {precision!r}")
        if precision == "f32" and sweep != "lattice":
            raise ValueError("WaveHoltz: precision 'f32' is an option of the lattice form; it needs sweep 'lattice'")
        if not isinstance(launch, str) or launch not in self.LAUNCHES:
            raise ValueError(f"WaveHoltz: launch must be 'sweep' or 'pair', not {launch!r}")
        if launch == "pair" and sweep != "lattice":
            raise ValueError("WaveHoltz: launch 'pair' is an option of the lattice form; it needs sweep 'lattice'")
        if cell_stiffness is not None:
            if sweep != "lattice":
                raise ValueError("WaveHoltz: cell_stiffness is an option of the lattice form; it needs sweep 'lattice'")
            if launch == "pair":
                raise ValueError("WaveHoltz: launch 'pair' has no form for cell_stiffness; it needs launch 'sweep'")
            try:
                cell_stiffness = np.asarray(cell_stiffness, dtype=np.float64)
            except (TypeError, ValueError):
                raise ValueError("WaveHoltz: cell_stiffness must be a one-dimensional array of floats") from None
            if cell_stiffness.ndim != 1:
                raise ValueError(f"WaveHoltz: cell_stiffness must be one-dimensional, one value per element, not of shape {cell_stiffness.shape}")
            cell_stiffness = np.ascontiguousarray(cell_stiffness)
            if not np.all(np.isfinite(cell_stiffness)) or not np.all(cell_stiffness > 0):
                raise ValueError("WaveHoltz: cell_stiffness must be finite and positive")
        if faces is not None:
            faces = np.asarray(faces)
            if faces.ndim != 1 or (faces.size and not np.issubdtype(faces.dtype, np.integer)):
                raise ValueError("WaveHoltz: faces must be a one-dimensional array of edge ids")
            faces = np.ascontiguousarray(faces, dtype=np.int32)
        h_a = np.ascontiguousarray(h_a, dtype=np.float64)
        if h_a.size != fem.size():
            raise ValueError(f"WaveHoltz: {h_a.size} coefficient values for {fem.size()} dofs")
        if not np.all(np.isfinite(h_a)) or not np.all(h_a > 0):
            raise ValueError("WaveHoltz: the coefficient a must be finite and positive")
        args = (float(omega), _h(h_a), fem._h, scheme, coarsen, ratio, self.STIFFNESS.index(stiffness), None if faces is None else _h(faces),
                -1 if faces is None else int(faces.size), self.SWEEPS.index(sweep))
        if cell_stiffness is not None:
            n_elem = fem.mesh.n_elem()
            if cell_stiffness.size != n_elem:
                raise ValueError(f"WaveHoltz: {cell_stiffness.size} cell_stiffness values for {n_elem} elements")
            h = lib.cuddh_waveholtz_create_cell_stiffness(*args, self.PRECISIONS.index(precision), self.LAUNCHES.index(launch), _h(cell_stiffness))
        elif launch != "sweep":
            h = lib.cuddh_waveholtz_create_launch(*args, self.PRECISIONS.index(precision), self.LAUNCHES.index(launch))
        elif precision == "f64":
            h = lib.cuddh_waveholtz_create_sweep(*args)
        else:
            h = lib.cuddh_waveholtz_create_precision(*args, self.PRECISIONS.index(precision))
        if not h and N.last_error().startswith("WaveHoltz error"):
            raise ValueError(f"WaveHoltz: {N.last_error()}")
        super().__init__(N.handle(h, "WaveHoltz"), (fem,), 2 * fem.size())
        self.fem, self.omega = fem, float(omega)

    @staticmethod
    def _integrator(integrator, coarsen):
        """(scheme, coarsen) of cuddh_waveholtz_create, or ValueError"""
        if not isinstance(integrator, str) or integrator not in ("rk2", "rk4"):
            raise ValueError(f"WaveHoltz: integrator must be 'rk2' or 'rk4', not {integrator!r}")
        if coarsen is None:
            coarsen = 1 if integrator == "rk2" else 4
        if isinstance(coarsen, (bool, np.bool_)) or not isinstance(coarsen, (int, np.integer)):
            raise ValueError(f"WaveHoltz: coarsen must be an integer in [1, 16], not {coarsen!r}")
        if not 1 <= coarsen <= 16:
            raise ValueError(f"WaveHoltz: coarsen must lie in [1, 16], got {int(coarsen)}")
        if integrator == "rk2" and coarsen != 1:
            raise ValueError("WaveHoltz: integrator 'rk2' marches on the mesh grid (coarsen 1) only; a coarser grid needs 'rk4'")
        return (0 if integrator == "rk2" else 1), int(coarsen)

    @staticmethod
    def _ratio(time_ratio) -> int:
        """time_ratio as cuddh_waveholtz_create takes it (0: from the coefficient), or ValueError"""
        if isinstance(time_ratio, str):
            if time_ratio != "coefficient":
                raise ValueError(f"WaveHoltz: time_ratio must be 'coefficient' or an integer in [1, 256], not {time_ratio!r}")
            return 0
        if isinstance(time_ratio, (bool, np.bool_)) or not isinstance(time_ratio, (int, np.integer)):
            raise ValueError(f"WaveHoltz: time_ratio must be 'coefficient' or an integer in [1, 256], not {time_ratio!r}")
        if not 1 <= time_ratio <= 256:
            raise ValueError(f"WaveHoltz: time_ratio must lie in [1, 256], got {int(time_ratio)}")
        return int(time_ratio)

    def size(self) -> int:
        return self._n

    def period(self, z_in, f, z_out):
        """z_out = W(z_in; f): one filtered period from z_in (None: zero) under the load f = [f_re; f_im] (None: none)"""
        N.check_capi(lib.cuddh_waveholtz_period(self._h, _ptr(z_in, "f64", self._n, "z_in"), _ptr(f, "f64", self._n, "f"),
                                                _ptr(z_out, "f64", self._n, "z_out")), "WaveHoltz.period")

    def rhs(self, f, b):
        self.period(None, f, b)

    def solution(self, z, u):
        """u = [z_u; z_v / omega]"""
        N.check_capi(lib.cuddh_waveholtz_solution(self._h, _ptr(z, "f64", self._n, "z"), _ptr(u, "f64", self._n, "u")), "WaveHoltz.solution")

    def info(self) -> dict:
        info = np.zeros(6, dtype=np.int32)
        dt = C.c_double()
        buf = C.create_string_buffer(160)
        N.check_capi(lib.cuddh_waveholtz_info(self._h, _h(info), C.byref(dt), buf, 160), "WaveHoltz.info")
        return {"nt": int(info[0]), "dt": dt.value, "ratio": int(info[1]), "integrator": "rk4" if info[2] else "rk2", "coarsen": int(info[3]),
                "sweeps_per_period": int(info[4]), "stiffness_kernel": buf.value.decode(),
                "sweep": self.SWEEPS[lib.cuddh_waveholtz_sweep(self._h)], "precision": self.PRECISIONS[lib.cuddh_waveholtz_precision(self._h)],
                "launch": self.LAUNCHES[lib.cuddh_waveholtz_launch(self._h)]}

    def solve(self, f, u, m: int = 20, maxit: int = 200, tol: float = 1e-6, orth: str = "mgs", augment: int = 0) -> "SolverOut":
        """rhs -> gmres from zero -> solution; u receives [Re U; Im U]"""
        import torch

        b = torch.empty(self._n, dtype=torch.float64, device=f.device)
        z = torch.zeros_like(b)
        self.rhs(f, b)
        out = gmres(self._n, z, self, b, m, maxit, tol, orth=orth, augment=augment)
        self.solution(z, u)
        return out


class WaveHoltzBox(_Operator):
    """Whole-domain WaveHoltz in three dimensions (csrc/include/cuddh/waveholtz_box.hpp): WaveHoltz's iteration for
    (K - w^2 M + i w H) U = f on the box box = ((ax, bx), (ay, by), (az, bz)) of shape = (nx, ny, nz) congruent brick elements
    with n_basis in [2, 8] Gauss-Lobatto points per direction; K the collocated stiffness, M = diag(a^2 m), H = diag(a h), one
    launch per Runge-Kutta sweep (csrc/kernels/wave_box.hip).  There is no 3-D mesh or space class: the box is described here.

    The lattice has Lx x Ly x Lz nodes, L = n (n_basis - 1) + 1 (lattice_shape()); every vector is 2 Lx Ly Lz float64, [u; v]
    with node (I, J, K) at I + Lx (J + Ly K), i.e. a (Lz, Ly, Lx) array flattened.  h_a: HOST coefficient of shape (Lz, Ly, Lx)
    or flat in that order, finite and positive.  nodes() gives the node coordinates, mass() the lumped mass m: the load of a
    nodal function g is m * g.  integrator, coarsen, time_ratio: WaveHoltz's, on the mesh size min(hx, hy, hz).  absorbing: the
    absorbing faces among "x0", "x1", "y0", "y1", "z0", "z1" (the others are sound-hard).
        W.rhs(f, b); gmres(W.size(), z, W, b, m, maxit, tol); W.solution(z, u)        (or W.solve(f, u, ...))
    precision "f64" (the default) or "f32" (DESIGN 4.5.7): the lattice vectors are stored and the sweeps computed in fp32
    (csrc/kernels/wave_box_f32.hip), half the march's memory and bytes per sweep.  z, f, b and the solution stay float64; y =
    x - S x is formed in float64.  It is meant for tolerances around 1e-4: the fp32 operator's own defect is about 1e-6 relative,
    so a solve to 1e-6 or below wants "f64".  info()["stiffness_kernel"] is then "wave_box nb<n> f32".
    Paired launches, missing cells and a per-cell stiffness exist in two dimensions only.
    Every argument error is a ValueError before any native call; a native refusal is a ValueError with its message."""

    FACES = ("x0", "x1", "y0", "y1", "z0", "z1")
    PRECISIONS = ("f64", "f32")

    def __init__(self, omega: float, h_a, shape, box, n_basis: int = 4, integrator: str = "rk2", coarsen: int | None = None, time_ratio=1,
                 absorbing=FACES, precision: str = "f64"):
        if not isinstance(precision, str) or precision not in self.PRECISIONS:
            raise ValueError(f"WaveHoltzBox: precision must be 'f64' or 'f32', not {precision!r}")
        scheme, coarsen = WaveHoltz._integrator(integrator, coarsen)
        ratio = WaveHoltz._ratio(time_ratio)
        if isinstance(omega, (bool, np.bool_)) or not isinstance(omega, (int, float, np.integer, np.floating)) or not np.isfinite(omega) or not omega > 0:
            raise ValueError(f"WaveHoltzBox: omega must be finite and positive, not {omega!r}")
        try:
            shape = tuple(shape)
        except TypeError:
            raise ValueError(f"WaveHoltzBox: shape must be (nx, ny, nz), not {shape!r}") from None
        if len(shape) != 3 or any(isinstance(n, (bool, np.bool_)) or not isinstance(n, (int, np.integer)) for n in shape):
            raise ValueError(f"WaveHoltzBox: shape must be three integers (nx, ny, nz), not {shape!r}")
        if any(n < 1 for n in shape):
            raise ValueError(f"WaveHoltzBox: every element count must be at least 1, not {shape!r}")
        if isinstance(n_basis, (bool, np.bool_)) or not isinstance(n_basis, (int, np.integer)) or not 2 <= n_basis <= 8:
            raise ValueError(f"WaveHoltzBox: n_basis must be an integer in [2, 8], not {n_basis!r}")
        try:
            box = np.ascontiguousarray(box, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("WaveHoltzBox: box must be ((ax, bx), (ay, by), (az, bz))") from None
        if box.shape != (3, 2) or not np.all(np.isfinite(box)) or not np.all(box[:, 0] < box[:, 1]):
            raise ValueError(f"WaveHoltzBox: box must be three finite intervals ((ax, bx), (ay, by), (az, bz)) with a < b, not {box.tolist()!r}")
        if isinstance(absorbing, str):
            raise ValueError(f"WaveHoltzBox: absorbing must be a sequence of face names among {self.FACES}, not {absorbing!r}")
        try:
            absorbing = tuple(absorbing)
        except TypeError:
            raise ValueError(f"WaveHoltzBox: absorbing must be a sequence of face names among {self.FACES}, not {absorbing!r}") from None
        if any(not isinstance(f, str) or f not in self.FACES for f in absorbing) or len(set(absorbing)) != len(absorbing):
            raise ValueError(f"WaveHoltzBox: absorbing must name distinct faces among {self.FACES}, not {absorbing!r}")
        mask = sum(1 << self.FACES.index(f) for f in absorbing)
        H = int(n_basis) - 1
        L = tuple(int(n) * H + 1 for n in shape)  # Lx, Ly, Lz
        rows = 4 if precision == "f32" else 2  # rows of the padded lattice hold a multiple of four floats or of two doubles
        stride = (L[0] + rows - 1) // rows * rows
        if stride * L[1] * L[2] > 0x7FFFFFFF:
            raise ValueError(f"WaveHoltzBox: the padded lattice of {stride} x {L[1]} x {L[2]} slots does not fit in an int")
        try:
            h_a = np.ascontiguousarray(h_a, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("WaveHoltzBox: h_a must be an array of floats") from None
        if h_a.shape not in ((L[2], L[1], L[0]), (L[0] * L[1] * L[2],)):
            raise ValueError(f"WaveHoltzBox: h_a must have shape {(L[2], L[1], L[0])} (Lz, Ly, Lx) or be flat in that order, not {h_a.shape}")
        if not np.all(np.isfinite(h_a)) or not np.all(h_a > 0):
            raise ValueError("WaveHoltzBox: the coefficient a must be finite and positive")
        args = (int(shape[0]), int(shape[1]), int(shape[2]), _h(box), int(n_basis), _h(h_a))
        if precision == "f64":
            h = lib.cuddh_waveholtz_box_create(float(omega), *args, scheme, coarsen, ratio, mask)
        else:
            h = lib.cuddh_waveholtz_box_create_precision(float(omega), *args, scheme, coarsen, ratio, mask, self.PRECISIONS.index(precision))
        if not h and N.last_error().startswith("WaveHoltz error"):
            raise ValueError(f"WaveHoltzBox: {N.last_error()}")
        n = L[0] * L[1] * L[2]
        super().__init__(N.handle(h, "WaveHoltzBox"), (), 2 * n)
        self.omega, self.shape, self.box, self.n_basis, self.absorbing = float(omega), tuple(int(n) for n in shape), box, int(n_basis), absorbing
        self._L, self._mask = L, mask

    def size(self) -> int:
        return self._n

    def lattice_shape(self) -> tuple:
        """(Lx, Ly, Lz), read from the native object"""
        dims = np.zeros(3, dtype=np.int32)
        N.check_capi(lib.cuddh_waveholtz_box_lattice(self._h, _h(dims)), "WaveHoltzBox.lattice_shape")
        return tuple(int(d) for d in dims)

    def nodes(self) -> np.ndarray:
        """HOST (Lz, Ly, Lx, 3): the coordinates (x, y, z) of every lattice node"""
        xi, _ = quadrature(self.n_basis)
        H = self.n_basis - 1
        lines = []
        for d in range(3):
            a, b = self.box[d]
            h = (b - a) / self.shape[d]
            i = np.arange(self._L[d])
            e = np.minimum(i // H, self.shape[d] - 1)
            lines.append(a + h * (e + 0.5 * (xi[i - e * H] + 1.0)))
        out = np.empty((self._L[2], self._L[1], self._L[0], 3))
        out[..., 0] = lines[0][None, None, :]
        out[..., 1] = lines[1][None, :, None]
        out[..., 2] = lines[2][:, None, None]
        return out

    def mass(self) -> np.ndarray:
        """HOST (Lz, Ly, Lx): the lumped mass m (without the coefficient); the load of a nodal function g is m * g"""
        m = np.empty(self._L[0] * self._L[1] * self._L[2])
        N.check_capi(lib.cuddh_wave_box_describe(*self.shape, _h(self.box), self.n_basis, None, self._mask, None, None, _h(m), None, None, None, None,
                                                 None), "WaveHoltzBox.mass")
        return m.reshape(self._L[2], self._L[1], self._L[0])

    def period(self, z_in, f, z_out):
        """z_out = W(z_in; f): one filtered period from z_in (None: zero) under the load f = [f_re; f_im] (None: none)"""
        N.check_capi(lib.cuddh_waveholtz_box_period(self._h, _ptr(z_in, "f64", self._n, "z_in"), _ptr(f, "f64", self._n, "f"),
                                                    _ptr(z_out, "f64", self._n, "z_out")), "WaveHoltzBox.period")

    def rhs(self, f, b):
        self.period(None, f, b)

    def solution(self, z, u):
        """u = [z_u; z_v / omega]"""
        N.check_capi(lib.cuddh_waveholtz_box_solution(self._h, _ptr(z, "f64", self._n, "z"), _ptr(u, "f64", self._n, "u")), "WaveHoltzBox.solution")

    def info(self) -> dict:
        info = np.zeros(6, dtype=np.int32)
        dt = C.c_double()
        buf = C.create_string_buffer(160)
        N.check_capi(lib.cuddh_waveholtz_box_info(self._h, _h(info), C.byref(dt), buf, 160), "WaveHoltzBox.info")
        return {"nt": int(info[0]), "dt": dt.value, "ratio": int(info[1]), "integrator": "rk4" if info[2] else "rk2", "coarsen": int(info[3]),
                "sweeps_per_period": int(info[4]), "nodes": int(info[5]), "stiffness_kernel": buf.value.decode(),
                "precision": self.PRECISIONS[lib.cuddh_waveholtz_box_precision(self._h)]}

    def solve(self, f, u, m: int = 20, maxit: int = 200, tol: float = 1e-6, orth: str = "mgs", augment: int = 0) -> "SolverOut":
        """rhs -> gmres from zero -> solution; u receives [Re U; Im U]"""
        import torch

        b = torch.empty(self._n, dtype=torch.float64, device=f.device)
        z = torch.zeros_like(b)
        self.rhs(f, b)
        out = gmres(self._n, z, self, b, m, maxit, tol, orth=orth, augment=augment)
        self.solution(z, u)
        return out


def _orth_code(orth) -> int:
    """the C API's code of an orthogonalisation name; anything but "mgs" / "cgs2" is a ValueError, before any native call"""
    if not isinstance(orth, str) or orth not in ORTHOGONALIZATIONS:
        raise ValueError(f"gmres: orth must be one of {sorted(ORTHOGONALIZATIONS)}, not {orth!r}")
    return ORTHOGONALIZATIONS[orth]


def _gmres_entry(name: str, code: int, head: tuple, res, h_res, h_time, augment: int = 0) -> int:
    """the entry point of the family `name` that takes these options, called: "mgs" without augmentation is `name` itself, another
    orthogonalisation `name`_orth (its code in front of the result), augment > 0 `name`_aug (code, then augment)"""
    suffix, options = ("_aug", (code, augment)) if augment > 0 else ("_orth", (code,)) if code != 0 else ("", ())
    return getattr(lib, name + suffix)(*head, *options, C.byref(res), _h(h_res), _h(h_time))


def _augment_count(augment, m) -> int:
    """augment as the C API takes it; anything but an integer in [0, m - 1] is a ValueError, before any native call"""
    if isinstance(augment, bool) or not isinstance(augment, (int, np.integer)):
        raise ValueError(f"gmres: augment must be an integer in [0, m - 1], not {augment!r}")
    if augment < 0 or (augment > 0 and augment >= m):
        raise ValueError(f"gmres: augment must be in [0, m - 1] = [0, {m - 1}], not {augment}")
    return int(augment)


ARITHMETICS = ("real", "complex")


def _check_arithmetic(arithmetic, n, A, Precond, reduce, orth, augment) -> bool:
    """True for "complex"; every combination gmres refuses under it is a ValueError here, before any native call"""
    if not isinstance(arithmetic, str) or arithmetic not in ARITHMETICS:
        raise ValueError(f"gmres: arithmetic must be one of {list(ARITHMETICS)}, not {arithmetic!r}")
    if arithmetic == "real":
        return False
    if n % 2 != 0:
        raise ValueError(f"gmres: arithmetic=\"complex\" reads the vectors as [Re; Im] and needs an even n, not {n}")
    if isinstance(A, _Operator) or Precond is not None:
        raise ValueError("gmres: arithmetic=\"complex\" takes a DDH or a callable operator and no preconditioner "
                         "(HelmholtzOperator is not complex-linear on [u; v])")
    if reduce is not None:
        raise ValueError("gmres: arithmetic=\"complex\" cannot be combined with reduce=")
    if orth != "mgs" or augment != 0:
        raise ValueError("gmres: arithmetic=\"complex\" needs orth=\"mgs\" and augment=0")
    return True


def gmres(n: int, x, A, b, m: int, maxit: int, tol: float = 1e-6, verbose: int = 0, max_seconds: float = 6 * 60 * 60, Precond=None,
          reduce=None, orth: str = "mgs", augment: int = 0, arithmetic: str = "real") -> SolverOut:
    """Restarted GMRES (reference include/gmres.hpp:33-36).  A: an operator of this module, a DDH,
    or a Python callable `A(x, y)` acting on device tensors of x's dtype.

    reduce (only with a callable A): `reduce(t)` sums the small device tensor `t` over all ranks in place
    (torch.distributed.all_reduce) -- the vectors are then partitioned over the processes, see dist.py.

    orth: how an Arnoldi step orthogonalises.  "mgs" (default, the reference's): modified Gram-Schmidt, one launch per basis vector
    and, with reduce=, k + 2 reductions of one scalar at step k.  "cgs2": classical Gram-Schmidt applied twice -- four launches
    and three reductions (of k + 1, k + 1 and 1 scalars) per step whatever k is, and a basis orthogonal to working precision (m <= 512).

    augment: 0 (default: restarted GMRES as above, bit for bit) or k in [1, m - 1]: LGMRES -- the last k corrections x_i - x_{i-1} take
    the place of the last Krylov columns of every cycle, so that information survives the restart.  Their images under A are
    differences of residuals the iteration has anyway: no operator application is added, a cycle with ka stored corrections
    applies A m - ka + 1 times, and 2 k more vectors are held.  Pays where restarting stalls (many subdomains across the domain,
    DESIGN 5.2); changes little where GMRES(m) already converges like full GMRES.  m <= 512.

    arithmetic: "real" (default: the iteration above, bit for bit) or "complex": x and b are read as n / 2 complex numbers, real parts
    in the first half and imaginary parts in the second -- the layout of a DDH trace vector [lambda; mu] -- and the iteration is
    GMRES(m) with complex inner products, Hessenberg matrix and Givens rotations.  m operator applications then minimise the
    residual over complex instead of real combinations of the Krylov vectors: twice the real dimensions from the same m + 1
    vectors, the same bytes and the same launches per step.  A must be complex-linear, A(i x) = i A(x) with i [a; b] = [-b; a]
    (check a callable with complex_linearity_defect).  DDH with exact local solves is so exactly; the time-stepped DDH with five
    WaveHoltz iterations is so to 3.9e-3 .. 6.2e-3 (fp64, a = 1, n_basis 4: 16 x 16 elements at omega = 3.2 pi, 32 x 32 at 6.4 pi and at
    2 pi), so the estimate inside a cycle is approximate there; convergence is decided, as always, by the true residual b - A x
    that ends every cycle.  Matvecs at a = 1, n_basis 4, GMRES(20), real against complex, from a numpy model of both iterations:
    exact local solves, 16 x 16 elements in 2 x 2-element subdomains, omega = pi, tol 1e-6: 551 against 141; time-stepped, 4 x 4-element
    subdomains: 16 x 16 at 3.2 pi, tol 1e-6: 109 against 68; 32 x 32 at 6.4 pi, tol 1e-6: 131 against 102; 32 x 32 at 2 pi, tol 1e-4: 248
    against 96.  Where GMRES(m) stalls (a cycle gains less than the operator misses complex linearity by) the true residual can RISE
    from cycle to cycle under "complex" -- measured on the 512 x 512, omega = 16 pi stall of DESIGN 5.2 -- so watch res_norm.
    Needs an even n, a DDH or a callable A, orth="mgs", augment=0, m <= 512; an _Operator (HelmholtzOperator
    anticommutes with i), Precond, reduce=, "cgs2" or augment > 0 under "complex" is a ValueError."""
    code = _orth_code(orth)
    aug = _augment_count(augment, m)
    aug_arg = (aug,) if aug else ()  # augment = 0 leaves the argument out: the call _gmres_entry has always had, which tests replace
    cplx = _check_arithmetic(arithmetic, n, A, Precond, reduce, orth, aug)
    import torch

    if reduce is not None and (isinstance(A, (DDH, _Operator)) or Precond is not None):
        raise ValueError("gmres: reduce= needs a callable operator and no preconditioner")

    res = N.SolverResult()
    h_res = np.zeros(maxit + 2)
    h_time = np.zeros(maxit + 2)
    if isinstance(A, DDH) and cplx:
        N.check_capi(lib.cuddh_gmres_ddh_cplx(n, _ptr(x, A.trace_dtype, n, "x"), A._h, _ptr(b, A.trace_dtype, n, "b"), m, maxit, float(tol), verbose, float(max_seconds),
                                              C.byref(res), _h(h_res), _h(h_time)), "gmres")
    elif isinstance(A, DDH):
        N.check_capi(_gmres_entry("cuddh_gmres_ddh", code, (n, _ptr(x, A.trace_dtype, n, "x"), A._h, _ptr(b, A.trace_dtype, n, "b"), m, maxit, float(tol), verbose, float(max_seconds)),
                                  res, h_res, h_time, *aug_arg), "gmres")
    elif isinstance(A, _Operator):
        N.check_capi(_gmres_entry("cuddh_gmres_f64", code, (n, _ptr(x, "f64", n, "x"), A._h, _ptr(b, "f64", n, "b"), Precond._h if Precond is not None else None, m, maxit,
                                                            float(tol), verbose, float(max_seconds)), res, h_res, h_time, *aug_arg), "gmres")
    else:
        dtype = x.dtype
        is64 = dtype == torch.float64
        dev = x.device
        errors = []

        views = {}

        def wrap(ptr, count):
            # view of library-owned device memory as a tensor (no copy); the solver reuses a handful of addresses
            key = (ptr, count)
            t = views.get(key)
            if t is None:
                t = views[key] = torch.as_tensor(_DevArray(ptr, count, is64), device=dev)
            return t

        def cb(ctx, xp, yp):
            try:
                A(wrap(xp, n), wrap(yp, n))
            except Exception as e:  # noqa: BLE001 - must not propagate through C
                errors.append(e)

        def red(ctx, sp, count, f64):
            try:
                reduce(wrap(sp, count))
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        cfun = N.ACTION_CB(cb)
        if cplx:
            N.check_capi(lib.cuddh_gmres_callback_cplx(n, _ptr(x, dtype, n, "x"), cfun, None, _ptr(b, dtype, n, "b"), int(is64), m, maxit, float(tol), verbose,
                                                       float(max_seconds), C.byref(res), _h(h_res), _h(h_time)), "gmres")
        elif reduce is None:
            N.check_capi(_gmres_entry("cuddh_gmres_callback", code, (n, _ptr(x, dtype, n, "x"), cfun, None, _ptr(b, dtype, n, "b"), int(is64), m, maxit, float(tol), verbose,
                                                                     float(max_seconds)), res, h_res, h_time, *aug_arg), "gmres")
        else:
            rfun = N.REDUCE_CB(red)
            N.check_capi(_gmres_entry("cuddh_gmres_callback_sharded", code, (n, _ptr(x, dtype, n, "x"), cfun, None, rfun, None, _ptr(b, dtype, n, "b"), int(is64), m, maxit,
                                                                             float(tol), verbose, float(max_seconds)), res, h_res, h_time, *aug_arg), "gmres")
        if errors:
            raise errors[0]
    return _solver_out(res, h_res, h_time)


def complex_linearity_defect(A, n: int, dtype, seed: int = 0) -> float:
    """|A(i x) - i A(x)| / |A x| on one random vector x of n entries read as [Re; Im], with i [a; b] = [-b; a]: how far the operator
    A (a DDH, or a callable `A(x, y)` on device tensors) is from complex-linear, at the cost of two applications.
    gmres(..., arithmetic="complex") assumes 0; a few 1e-3 (the time-stepped DDH) only makes its in-cycle estimate approximate.
    dtype: a torch dtype or "f32" / "f64" (a DDH applies in its own trace dtype, which must be this one)."""
    import torch

    if n < 2 or n % 2 != 0:
        raise ValueError(f"complex_linearity_defect: n must be even and positive, not {n}")
    dt = {"f32": torch.float32, "f64": torch.float64}.get(dtype, dtype)
    if dt not in (torch.float32, torch.float64):
        raise ValueError(f"complex_linearity_defect: dtype must be float32 or float64, not {dtype!r}")
    if isinstance(A, DDH) and A.trace_dtype != dt:
        raise ValueError(f"complex_linearity_defect: this DDH applies in {A.trace_dtype}, not {dt}")
    apply = A.action if isinstance(A, DDH) else A
    h = n // 2
    g = torch.Generator(device="cpu").manual_seed(int(seed))
    x = torch.randn(n, dtype=torch.float64, generator=g).to(dt).cuda()
    ix = torch.cat([-x[h:], x[:h]])
    y, z = torch.zeros_like(x), torch.zeros_like(x)
    apply(x, y)
    apply(ix, z)
    iy = torch.cat([-y[h:], y[:h]])
    return float(torch.linalg.norm((z - iy).double()) / torch.linalg.norm(y.double()))


class _DevArray:
    """Minimal __cuda_array_interface__ carrier so torch can view library-owned device memory."""

    def __init__(self, ptr: int, count: int, is64: bool):
        self.__cuda_array_interface__ = {
            "shape": (count,),
            "typestr": "<f8" if is64 else "<f4",
            "data": (int(ptr), False),
            "version": 2,
        }
