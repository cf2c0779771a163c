"""The patch layout every plan kernel of csrc/kernels/helmholtz_fused.hip trusts (csrc/src/patch_layout.cpp): element order,
patch-local numbering, colours, border slots and the plan-native ordering, read back through cuddh_patch_layout_* and checked in
numpy on the arrays alone.  Host code: no GPU."""
import ctypes as C
import functools

import numpy as np
import pytest

import cuddhelmholtz_amd as cd
from cuddhelmholtz_amd._native import lib

import irregular_meshes
from conftest import GOLDEN

INT_ARRAYS = ("perm", "dof_off", "dof_list", "slot_of", "own_count", "patch_nel", "face_off", "face_id", "shared_dof", "shared_off", "own_off", "bpos",
              "bslot", "global_of_native")
OTHER_ARRAYS = {"lidx": np.uint32, "face_lidx": np.uint16, "colour": np.uint8, "face_col": np.uint8, "dest_entries": np.int64}
SCALARS = ("pe", "n_patches", "dof_stride", "max_loc", "ncol", "nfcol", "n_shared", "n_slots", "has_native", "n_owned", "bstride", "list_entries",
           "owned_entries", "native_list_entries")


def build_layout(ndof, nb, I, xy, fI, face_elem, pe, fused, fixed_stride):
    """(error code, {name: array or int}) of cuddh_patch_layout_create on HOST arrays: I (nb*nb, n_elem), fI (nb, n_faces)"""
    I = np.asfortranarray(I, dtype=np.int32)
    n_elem = I.shape[-1]
    n_faces = 0 if fI is None else fI.shape[-1]
    keep = [I]
    ptr = lambda a, dt: None if a is None else keep.append(np.asfortranarray(a, dtype=dt)) or keep[-1].ctypes.data  # noqa: E731
    h = C.c_void_p()
    err = lib.cuddh_patch_layout_create(C.byref(h), ndof, n_elem, nb, I.ctypes.data, ptr(None if xy is None else xy.T, np.float64), n_faces,
                                        ptr(fI, np.int32), ptr(face_elem, np.int32), pe, int(fused), int(fixed_stride))
    if err:
        assert not h.value
        return err, None
    try:
        out = {}
        for name, dt in [(n, np.int32) for n in INT_ARRAYS] + list(OTHER_ARRAYS.items()) + [(n, np.int64) for n in SCALARS]:
            count = lib.cuddh_patch_layout_array(h, name.encode(), None, 1)
            assert count >= 0, name
            a = np.empty(count, dtype=dt)
            assert lib.cuddh_patch_layout_array(h, name.encode(), a.ctypes.data, 0) == count
            out[name] = int(a[0]) if name in SCALARS else a
        assert lib.cuddh_patch_layout_array(h, b"no such field", None, 1) == -1
        return 0, out
    finally:
        lib.cuddh_patch_layout_destroy(h)


@functools.lru_cache(maxsize=None)
def mesh_of(name):
    if "(" in name:  # generated: tests/irregular_meshes.py
        return cd.Mesh2D.from_vertices(*irregular_meshes.by_name(name))
    if name.startswith("rect"):
        n = int(name[4:])
        return cd.Mesh2D.uniform_rect(n, -1.0, 1.0, n, -1.0, 1.0)
    mesh = cd.Mesh2D.load(GOLDEN / "unstructured_square")
    return mesh.refined(2) if name == "unstructured refined twice" else mesh


@functools.lru_cache(maxsize=None)
def space_of(mesh_name, nb):
    """the arrays HelmholtzOperator hands to plan creation, from the public classes"""
    mesh = mesh_of(mesh_name)
    fem = cd.H1Space(mesh, cd.Basis(nb))
    I = fem.global_indices().reshape(nb * nb, -1, order="F")
    xy = mesh.vertices()[mesh.elements()].mean(axis=1)  # (n_elem, 2) centroids
    faces = mesh.boundary_edges()
    fs = cd.FaceSpace(fem, faces)
    fI = fs.global_indices()[fs.subspace_indices()]  # (nb, n_faces) face node -> H1 dof
    face_elem = mesh.edges()[faces, 3]
    return fem.size(), I, xy, fI, face_elem


MESHES = ("rect1", "rect10", "rect37", "unstructured", "unstructured refined twice", "star(8,4,0.0785,2.0)", "star(6,9,0.6283)", "star(3,2)", "annulus(3,1)",
          "annulus(7,2)", "l_shape(6)")
ORDERS = ((2, 32), (2, 64), (4, 32), (4, 64), (5, 32), (5, 64), (6, 16), (8, 16))  # (n_basis, elements per patch)
VARIANTS = [(fused, fixed) for fused in (True, False) for fixed in (True, False)]  # (fused or single-operator, fixed stride)


class Case:
    """one layout with its inputs and what numpy derives from the inputs and the permutation alone"""

    def __init__(self, mesh_name, nb, pe, fused, fixed):
        self.ndof, self.I, xy, fI, face_elem = space_of(mesh_name, nb)
        self.nb, self.pe, self.fused, self.fixed = nb, pe, fused, fixed
        self.fI, self.face_elem = (fI, face_elem) if fused else (None, None)  # the single operators have no boundary term
        self.n_elem = self.I.shape[1]
        err, L = build_layout(self.ndof, nb, self.I, xy, self.fI, self.face_elem, pe, fused, fixed)
        assert err == 0
        self.L = L
        self.P = P = L["n_patches"]
        assert L["pe"] == pe and P == -(-self.n_elem // pe)
        self.n_loc = np.diff(L["dof_off"])
        # the start of patch q's segment of dof_list / slot_of
        self.start = np.arange(P) * L["dof_stride"] if L["dof_stride"] else L["dof_off"][:-1]

    def segment(self, name, q):
        return self.L[name][self.start[q]:self.start[q] + self.n_loc[q]]

    @functools.cached_property
    def touches(self):
        """how many patches touch each dof, from I and the permutation"""
        perm = self.L["perm"][:self.n_elem]
        patch = np.repeat(np.arange(self.n_elem) // self.pe, self.I.shape[0])
        pairs = np.unique(np.stack([self.I[:, perm].T.ravel(), patch]), axis=1)
        return np.bincount(pairs[0], minlength=self.ndof)


@functools.lru_cache(maxsize=None)
def case(mesh_name, nb, pe, fused, fixed):
    return Case(mesh_name, nb, pe, fused, fixed)


def cases(mesh_name, nb, pe):
    return [case(mesh_name, nb, pe, fused, fixed) for fused, fixed in VARIANTS]


def layouts(f):
    return pytest.mark.parametrize("mesh_name", MESHES)(pytest.mark.parametrize("nb,pe", ORDERS)(f))


@layouts
def test_permutation_and_list_shapes(mesh_name, nb, pe):
    for c in cases(mesh_name, nb, pe):
        L = c.L
        perm = L["perm"]
        assert perm.size == c.P * pe
        assert np.array_equal(np.sort(perm[:c.n_elem]), np.arange(c.n_elem))  # every element once
        assert np.all(perm[c.n_elem:] == -1)
        assert np.array_equal(L["patch_nel"], np.minimum(pe, c.n_elem - pe * np.arange(c.P)))
        assert L["dof_off"][0] == 0 and L["max_loc"] == c.n_loc.max() and L["list_entries"] == L["dof_off"][-1]
        if c.fixed:  # padded lists repeat their last entry up to max_loc
            assert L["dof_stride"] == L["max_loc"]
            for name in ("dof_list", "slot_of"):
                rows = L[name].reshape(c.P, L["max_loc"])
                for q in range(c.P):
                    assert np.all(rows[q, c.n_loc[q]:] == rows[q, c.n_loc[q] - 1])
        else:
            assert L["dof_stride"] == 0 and L["dof_list"].size == L["slot_of"].size == L["dof_off"][-1]


@layouts
def test_owned_first_border_last_and_slots(mesh_name, nb, pe):
    for c in cases(mesh_name, nb, pe):
        L = c.L
        shared = L["shared_dof"]
        assert np.array_equal(np.sort(shared), np.flatnonzero(c.touches > 1)) and np.unique(shared).size == shared.size
        assert np.array_equal(np.diff(L["shared_off"]), c.touches[shared]) and L["shared_off"][0] == 0
        assert L["n_shared"] == shared.size and L["n_slots"] == L["shared_off"][-1]
        slots, slot_patch, slot_dof = [], [], []
        for q in range(c.P):
            dofs, dest, own = c.segment("dof_list", q), c.segment("slot_of", q), L["own_count"][q]
            assert np.unique(dofs).size == dofs.size  # no repeats
            assert np.all(c.touches[dofs[:own]] == 1) and np.all(c.touches[dofs[own:]] > 1)  # owned: touched by no other patch
            assert np.array_equal(dest[:own], dofs[:own])  # owned: the dof itself
            assert np.all(dest[own:] < 0)  # border: -(slot) - 1
            slots.append(-dest[own:] - 1)
            slot_patch.append(np.full(dofs.size - own, q))
            slot_dof.append(dofs[own:])
        slots, slot_patch, slot_dof = map(np.concatenate, (slots, slot_patch, slot_dof))
        order = np.argsort(slots, kind="stable")
        assert np.array_equal(slots[order], np.arange(L["n_slots"]))  # every slot exactly once
        # the slots of border dof j are shared_off[j] .. shared_off[j+1], in increasing patch order
        assert np.array_equal(slot_dof[order], np.repeat(shared, np.diff(L["shared_off"])))
        same_dof = np.diff(slot_dof[order]) == 0
        assert np.all(np.diff(slot_patch[order])[same_dof] > 0)
        assert L["owned_entries"] == L["own_count"].sum() and L["native_list_entries"] == (c.n_loc - L["own_count"]).sum()
        for k, row in ((1, 64), (2, 128)):
            assert L["dest_entries"][k] == c.P + (c.n_loc - L["own_count"] // row * row).sum()
        assert L["dest_entries"][0] == L["dof_off"][-1]
    if mesh_name == "rect1":
        assert L["n_shared"] == 0 and L["n_slots"] == 0


@layouts
def test_lidx_reproduces_the_index_map(mesh_name, nb, pe):
    nn = nb * nb
    for c in cases(mesh_name, nb, pe):
        lidx = c.L["lidx"].reshape(c.P, (nn + 1) // 2, pe)
        for q in range(c.P):
            nel = c.L["patch_nel"][q]
            local = np.stack([(lidx[q, n // 2, :nel] >> (16 * (n & 1))) & 0xFFFF for n in range(nn)])  # (nn, nel)
            assert local.max() < c.n_loc[q]
            assert np.array_equal(c.segment("dof_list", q)[local], c.I[:, c.L["perm"][q * pe:q * pe + nel]])
            assert np.all(lidx[q, :, nel:] == 0)


def assert_colours_separate(local, colours):
    """local (n_items, n_nodes) patch-local dofs, colours (n_items): two items of one colour share no dof"""
    keys = colours.astype(np.int64)[:, None] * 65536 + local
    assert np.unique(keys).size == keys.size


@layouts
def test_colours(mesh_name, nb, pe):
    nn = nb * nb
    for c in cases(mesh_name, nb, pe):
        L = c.L
        lidx, colour = L["lidx"].reshape(c.P, (nn + 1) // 2, pe), L["colour"].reshape(c.P, pe)
        top = 0
        for q in range(c.P):
            nel = L["patch_nel"][q]
            local = np.stack([(lidx[q, n // 2, :nel] >> (16 * (n & 1))) & 0xFFFF for n in range(nn)], axis=1).astype(np.int64)
            assert_colours_separate(local, colour[q, :nel])
            top = max(top, colour[q, :nel].max())
            t0, t1 = L["face_off"][q], L["face_off"][q + 1]
            assert_colours_separate(L["face_lidx"].reshape(-1, nb)[t0:t1].astype(np.int64), L["face_col"][t0:t1])
        assert L["ncol"] == top + 1 <= 31
        if c.fused:
            assert L["nfcol"] == L["face_col"].max() + 1 <= 31
        else:
            assert L["nfcol"] == 0 and L["face_col"].size == 0 and np.all(L["face_off"] == 0)


@layouts
def test_faces(mesh_name, nb, pe):
    for c in cases(mesh_name, nb, pe):
        if not c.fused:
            continue
        L = c.L
        n_faces = c.fI.shape[1]
        assert np.array_equal(np.sort(L["face_id"]), np.arange(n_faces)) and L["face_off"][-1] == n_faces
        patch_of_elem = np.empty(c.n_elem, dtype=np.int64)
        patch_of_elem[L["perm"][:c.n_elem]] = np.arange(c.n_elem) // pe
        face_lidx = L["face_lidx"].reshape(n_faces, nb)
        for q in range(c.P):
            t = slice(L["face_off"][q], L["face_off"][q + 1])
            assert np.all(patch_of_elem[c.face_elem[L["face_id"][t]]] == q)  # grouped by the patch of their element
            assert np.array_equal(c.segment("dof_list", q)[face_lidx[t]], c.fI[:, L["face_id"][t]].T)  # every face node -> its global dof


@layouts
def test_native_ordering(mesh_name, nb, pe):
    for c in cases(mesh_name, nb, pe):
        L = c.L
        if not c.fused:  # the single operators take vectors in the reference ordering only
            assert L["has_native"] == 0 and all(L[n].size == 0 for n in ("own_off", "bpos", "bslot", "global_of_native"))
            continue
        assert L["has_native"] == 1
        assert np.array_equal(np.sort(L["global_of_native"]), np.arange(c.ndof))  # a permutation
        assert np.array_equal(L["own_off"], np.concatenate([[0], np.cumsum(L["own_count"])]))
        n_owned, bstride = L["n_owned"], L["bstride"]
        assert n_owned == L["own_off"][-1] and bstride == max(1, (c.n_loc - L["own_count"]).max())
        index_in_shared = np.full(c.ndof, -1)
        index_in_shared[L["shared_dof"]] = np.arange(L["n_shared"])
        bpos, bslot = L["bpos"].reshape(c.P, bstride), L["bslot"].reshape(c.P, bstride)
        for q in range(c.P):
            own = L["own_count"][q]
            dofs, dest = c.segment("dof_list", q), c.segment("slot_of", q)
            assert np.array_equal(L["global_of_native"][L["own_off"][q]:L["own_off"][q + 1]], dofs[:own])
            n_border = dofs.size - own
            if n_border == 0:
                continue
            assert np.array_equal(bpos[q, :n_border], n_owned + index_in_shared[dofs[own:]])  # border dofs in local order
            assert np.array_equal(bslot[q, :n_border], -dest[own:] - 1)
            assert np.array_equal(L["global_of_native"][bpos[q, :n_border]], dofs[own:])
            assert np.all(bpos[q, n_border:] == bpos[q, n_border - 1]) and np.all(bslot[q, n_border:] == bslot[q, n_border - 1])
        if mesh_name == "rect1":
            assert bstride == 1 and L["n_shared"] == 0


# ---- fabricated connectivities, no mesh
def star(n_elem):
    """n_elem four-node elements (n_basis 2) that all contain dof 0"""
    I = np.zeros((4, n_elem), dtype=np.int32)
    I[1:] = 1 + np.arange(3 * n_elem).reshape(n_elem, 3).T
    return 1 + 3 * n_elem, I


@pytest.mark.parametrize("fused", (True, False))
def test_a_32nd_colour_is_refused(fused):
    ndof, I = star(33)
    assert build_layout(ndof, 2, I, None, None, None, 64, fused, True)[0] == 801  # hipErrorNotSupported: callers fall back


def test_31_elements_at_one_dof_take_31_colours():
    ndof, I = star(31)
    err, L = build_layout(ndof, 2, I, None, None, None, 64, True, True)
    assert err == 0 and L["ncol"] == 31
    assert np.array_equal(np.sort(L["colour"][:31]), np.arange(31))


def test_32_faces_at_one_dof_are_refused():
    # one element holds every dof; its 32 two-node "faces" all contain dof 0
    I = np.arange(4, dtype=np.int32).reshape(4, 1)
    fI = np.stack([np.zeros(32, dtype=np.int32), 1 + np.arange(32, dtype=np.int32) % 3])
    assert build_layout(4, 2, I, None, fI, np.zeros(32, dtype=np.int32), 64, True, True)[0] == 801
    err, L = build_layout(4, 2, I, None, fI[:, :31], np.zeros(31, dtype=np.int32), 64, True, True)
    assert err == 0 and L["nfcol"] == 31


def test_face_dof_outside_its_elements_patch_is_an_error():
    # 33 disjoint elements in patches of 32: element 32 is alone in patch 1, the face names it but holds dofs of element 0
    I = np.arange(4 * 33, dtype=np.int32).reshape(33, 4).T
    fI = np.array([[0], [1]], dtype=np.int32)
    assert build_layout(4 * 33, 2, I, None, fI, np.array([32], dtype=np.int32), 32, True, True)[0] == 1  # hipErrorInvalidValue
    assert build_layout(4 * 33, 2, I, None, fI, np.array([0], dtype=np.int32), 32, True, True)[0] == 0
