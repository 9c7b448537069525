"""Grid projection: drop-in for the reference's ``Projection`` (processing/projection.py) and the coordinate / grid handling
of its ``DataProcessor`` (stream/data_processor.py:83-139,162-236,292-294,313-337).

``GridProjection`` is the HOST plan, in float64 with the reference's arithmetic and quirks: the coordinates of the four
regions, the grids, the projection matrices, the active grid points and the projected channels are fixed when it is built;
``layout(keys)`` resolves the key names of one stream (which columns are feature f of projected channel k, what the grid keys
are called and where they go) the way ``Projection.init_projection_run`` does at the first hop.  ``DeviceProjection`` runs the
per-hop product on the GPU (nmx_k_proj.h): inside the engine's launch sequence (``nmx_plan_attach_proj``), or on a table of
rows (user features, ragged runs).
"""

from __future__ import annotations

import importlib.util
from pathlib import Path, PurePath

import numpy as np

REGIONS = [f"{loc}_{lat}" for loc in ("cortex", "subcortex") for lat in ("left", "right")]


def add_coordinates(coord_names, coord_list) -> dict:
    """DataProcessor._add_coordinates (stream/data_processor.py:93-139): a coordinate goes to a cortex region when its name
    contains "ECOG", to a subcortex region when it contains "LFP" (case-sensitive substring tests); left is x < 0, right
    x > 0; positions * 1000."""
    coords: dict = {}
    for region in REGIONS:
        left = region.split("_")[1] == "left"
        kind = "ECOG" if region.split("_")[0] == "cortex" else "LFP"

        def here(val) -> bool:
            return val < 0 if left else val > 0

        coords[region] = {"ch_names": [n for n, c in zip(coord_names, coord_list) if here(c[0]) and kind in n]}
        positions = [c for c, n in zip(coord_list, coord_names) if here(c[0]) and kind in n]
        coords[region]["positions"] = np.array(positions, dtype=np.float64) * 1000
    return coords


def grid_dir(path_grids) -> Path:
    """``path_grids``, or the directory of an installed reference package (found without importing it)."""
    if path_grids is not None:
        return Path(path_grids)
    spec = importlib.util.find_spec("py_neuromodulation")
    if spec is None or not spec.origin:
        raise FileNotFoundError("grid projection needs the grid files grid_cortex.tsv / grid_subcortex.tsv: pass "
                                "path_grids (no installed py_neuromodulation package to take them from)")
    return Path(spec.origin).parent


def read_grid(path_grids, grid_str: str):
    """io.read_grid (utils/io.py:152-175): ``{dir}/grid_{cortex|subcortex}.tsv``, tab separated."""
    import pandas as pd

    return pd.read_csv(PurePath(grid_dir(path_grids), "grid_" + grid_str.lower() + ".tsv"), sep="\t")


def calc_proj_matrix(max_dist: float, grid: np.ndarray, coord_array: np.ndarray) -> np.ndarray:
    """Projection.calc_proj_matrix (:105-133): grid[3, n_points], coord_array[n_contacts, 3] -> [n_points, n_contacts],
    row g = (1 / d) / sum(1 / d) over the contacts with d < max_dist (zero row without any)."""
    # (np.linalg.norm pair by pair, as the reference: the sidecar carries these matrices, bit for bit)
    dist = np.zeros([grid.shape[1], coord_array.shape[0]])
    for g in range(grid.shape[1]):
        for c in range(coord_array.shape[0]):
            dist[g, c] = np.linalg.norm(grid[:, g] - coord_array[c, :])
    proj = np.zeros(dist.shape)
    for g in range(dist.shape[0]):
        used = np.where(dist[g, :] < max_dist)[0]
        rec = dist[g, used]
        proj[g, used] = (1 / dist[g, used]) / np.sum(1 / rec)
    return proj


class GridProjection:
    """Projection.__init__ (processing/projection.py:16-90) of one stream.  Raises what the reference raises while its
    DataProcessor is built: AttributeError without coordinates (``self.coords``), with ECoG coordinates on both hemispheres
    (``sess_right``) and for ``project_subcortex`` without LFP coordinates on the session's side (``lfp_elec_names``)."""

    def __init__(self, settings, channels, coord_names=None, coord_list=None, path_grids=None) -> None:
        pp = settings.postprocessing
        self.project_cortex = bool(pp.project_cortex)
        self.project_subcortex = bool(pp.project_subcortex)
        self.max_dist_cortex = float(settings.project_cortex_settings.max_dist_mm)
        self.max_dist_subcortex = float(settings.project_subcortex_settings.max_dist_mm)
        coords = add_coordinates(coord_names, coord_list) if (coord_list is not None and coord_names is not None) else None
        # DataProcessor._get_projection: the grids are read, then the coordinates handed over
        self.grid_cortex = read_grid(path_grids, "cortex") if self.project_cortex else None
        self.grid_subcortex = read_grid(path_grids, "subcortex") if self.project_subcortex else None
        if coords is None:
            raise AttributeError("'DataProcessor' object has no attribute 'coords'")
        self.coords = coords
        self.channels = channels
        self._remove_not_used_ch_from_coords()
        if len(coords["cortex_left"]["positions"]) == 0:
            self.sess_right = True
            self.ecog_strip, self.ecog_strip_names = coords["cortex_right"]["positions"], coords["cortex_right"]["ch_names"]
        elif len(coords["cortex_right"]["positions"]) == 0:
            self.sess_right = False
            self.ecog_strip, self.ecog_strip_names = coords["cortex_left"]["positions"], coords["cortex_left"]["ch_names"]
        else:
            raise AttributeError("'Projection' object has no attribute 'sess_right'")
        side = "right" if self.sess_right else "left"
        if len(coords[f"subcortex_{side}"]["positions"]) > 0:
            self.lfp_elec = coords[f"subcortex_{side}"]["positions"]
            self.lfp_elec_names = coords[f"subcortex_{side}"]["ch_names"]
        self.ecog_channels: list[str] = []
        self.lfp_channels: list[str] = []
        self._initialize_channels()
        self.proj_matrix_cortex, self.proj_matrix_subcortex = self._calc_projection_matrix()
        self.active_cortex_gridpoints = (np.nonzero(self.proj_matrix_cortex.sum(axis=1))[0] if self.project_cortex
                                         else np.zeros(0, np.int64))
        self.active_subcortex_gridpoints = (np.nonzero(self.proj_matrix_subcortex.sum(axis=1))[0] if self.project_subcortex
                                            else np.zeros(0, np.int64))
        self._layouts: dict = {}

    def _remove_not_used_ch_from_coords(self) -> None:
        """:92-103 as it is: ``startswith`` match, deletion while iterating (the entry behind a deleted one is skipped),
        ``ch_names.remove(ch)`` of the CHANNEL's name."""
        ch = self.channels
        not_used = ch["name"][(ch["used"] == 0) | (ch["status"] == "bad")]
        for name in not_used:
            for key in self.coords:
                names = self.coords[key]["ch_names"]
                for idx, ch_coords in enumerate(names):
                    if name.startswith(ch_coords):
                        self.coords[key]["positions"] = np.delete(self.coords[key]["positions"], idx, axis=0)
                        names.remove(name)

    def _names_of(self, query_mask, allowed) -> list[str]:
        ch = self.channels
        names = ch["name"][query_mask].to_list()
        names = [n for n in names if n in allowed]
        return ch["new_name"][ch["name"].isin(names)].to_list()

    def _initialize_channels(self) -> None:
        """:195-226: used, good ECoG / (lfp, seeg, dbs) channels named in the coordinates, as new_name in table order."""
        ch = self.channels
        good = (ch["used"] == 1) & (ch["status"] == "good")
        if self.project_cortex:
            self.ecog_channels = self._names_of(good & (ch["type"] == "ecog"), self.ecog_strip_names)
        if self.project_subcortex:
            self.lfp_channels = self._names_of(good & ch["type"].isin(["lfp", "seeg", "dbs"]), self.lfp_elec_names)

    def _calc_projection_matrix(self):
        """:135-193: the grids of a right session mirrored (x -> -x)."""
        out = [None, None]
        for i, (on, grid, dist) in enumerate([(self.project_cortex, self.grid_cortex, self.max_dist_cortex),
                                              (self.project_subcortex, self.grid_subcortex, self.max_dist_subcortex)]):
            if not on:
                continue
            g = np.array(grid, dtype=np.float64)
            if self.sess_right:
                g[:, 0] = g[:, 0] * -1
            coord_array = self.ecog_strip if i == 0 else self.lfp_elec
            out[i] = calc_proj_matrix(dist, g.T, coord_array)
        return out[0], out[1]

    # ---- the first hop (init_projection_run, :228-278) -------------------------------------------------------------------
    def layout(self, keys) -> "ProjectionLayout":
        """The key names of one stream -> where the projection reads and writes (cached per key list)."""
        keys = list(keys)
        tok = tuple(keys)
        lay = self._layouts.get(tok)
        if lay is None:
            lay = self._layouts[tok] = ProjectionLayout(self, keys)
        return lay

    def sidecar(self) -> dict:
        """stream/data_processor.py:326-333: what the projection adds to the sidecar."""
        out: dict = {"coords": self.coords}
        if self.project_cortex:
            out["grid_cortex"] = self.grid_cortex
            out["proj_matrix_cortex"] = self.proj_matrix_cortex
        if self.project_subcortex:
            out["grid_subcortex"] = self.grid_subcortex
            out["proj_matrix_subcortex"] = self.proj_matrix_subcortex
        return out


class ProjectionLayout:
    """One key list resolved: ``gather[k, f]`` (the column of feature f of projected channel k: ECoG channels, then LFP),
    the sparse weights of every active point, the grid keys (``gridcortex_{g}_{feature}``, then ``gridsubcortex_...``; the
    features outer, the active points inner) and their columns: the grid columns follow the ``len(keys)`` columns of the
    key list (dict.update of new keys).  Raises the reference's ValueError for ragged channels (a ``new_name`` that is a
    prefix of another channel's keys) and its matmul ValueError when the projected channels and the contacts differ in number."""

    def __init__(self, plan: GridProjection, keys: list[str]) -> None:
        self.n_keys = len(keys)
        groups = []   # (rows of gather, matrix, active points, key prefix)
        feature_names = None
        if plan.project_cortex:
            rows = [[i for i, k in enumerate(keys) if k.startswith(ch)] for ch in plan.ecog_channels]
            if rows:
                feature_names = [keys[i][len(plan.ecog_channels[0]) + 1:] for i in rows[0]]
            groups.append((rows, plan.proj_matrix_cortex, plan.active_cortex_gridpoints, "gridcortex_"))
        if plan.project_subcortex:
            rows = [[i for i, k in enumerate(keys) if k.startswith(ch)] for ch in plan.lfp_channels]
            if not feature_names and rows:
                feature_names = [keys[i][len(plan.lfp_channels[0]) + 1:] for i in rows[0]]
            groups.append((rows, plan.proj_matrix_subcortex, plan.active_subcortex_gridpoints, "gridsubcortex_"))
        if feature_names is None:   # (no projected channel at all: the reference iterates over None)
            raise TypeError("'NoneType' object is not iterable")
        self.feature_names = feature_names
        F = len(feature_names)
        gather, ptr, idx, w, out_col, out_stride, point_group, group_chan = [], [0], [], [], [], [], [], [0]
        self.grid_keys: list[str] = []
        col = self.n_keys
        ch0 = 0
        for rows, P, active, prefix in groups:
            lens = {len(r) for r in rows}
            if len(lens) > 1:   # np.array of ragged lists (projection.py:286-306)
                raise ValueError("setting an array element with a sequence. The requested array has an inhomogeneous "
                                 f"shape after 1 dimensions ({prefix[:-1]}: projected channels with {sorted(lens)} keys)")
            n_f = lens.pop() if lens else 0
            if P.shape[1] != len(rows):   # P @ X
                raise ValueError(f"matmul: Input operand 1 has a mismatch in its core dimension 0 (size {len(rows)} is "
                                 f"different from {P.shape[1]}): {prefix[:-1]} has {P.shape[1]} contacts and "
                                 f"{len(rows)} projected channels")
            if len(active) and F > n_f:   # proj_array[g, feature_idx] beyond the group's features
                raise IndexError(f"index {n_f} is out of bounds for axis 1 with size {n_f}")
            gather += [r[:F] for r in rows]
            G = len(active)
            for gi, g in enumerate(active):
                nz = np.nonzero(P[g])[0]
                idx += [ch0 + int(k) for k in nz]
                w += [float(P[g, k]) for k in nz]
                ptr.append(len(idx))
                out_col.append(col + gi)
                out_stride.append(G)
                point_group.append(len(group_chan) - 1)
            self.grid_keys += [f"{prefix}{g}_{name}" for name in feature_names for g in active]
            col += G * F
            ch0 += len(rows)
            group_chan.append(ch0)
        self.groups = groups
        self.n_grid = col - self.n_keys
        self.n_feat = F
        self.gather = np.array(gather, dtype=np.int32).reshape(ch0, F)
        self.ptr = np.array(ptr, dtype=np.int32)
        self.idx = np.array(idx, dtype=np.int32)
        self.w = np.array(w, dtype=np.float64)
        self.out_col = np.array(out_col, dtype=np.int32)
        self.out_stride = np.array(out_stride, dtype=np.int32)
        self.point_group = np.array(point_group, dtype=np.int32)
        self.group_chan = np.array(group_chan, dtype=np.int32)

    @property
    def empty(self) -> bool:
        """Nothing to compute (no active point or no feature): the grid keys, if any, are all there is."""
        return self.n_grid == 0 or len(self.gather) == 0

    def project(self, table: np.ndarray) -> np.ndarray:
        """The float64 reference of the device kernel: ``table[n, >= n_keys]`` -> float64 [n, n_grid], hop by hop the
        reference's dense products P @ X of every group, its active points in key order (features outer)."""
        out = np.empty((table.shape[0], self.n_grid))
        c0 = 0
        col = 0
        for rows, P, active, _ in self.groups:
            k1 = c0 + len(rows)
            G = len(active)
            for i in range(table.shape[0]):
                X = table[i][self.gather[c0:k1]]          # [C_group, F]
                Y = P @ X
                out[i, col:col + G * self.n_feat] = Y[active].T.reshape(-1)
            col += G * self.n_feat
            c0 = k1
        return out


class DeviceProjection:
    """One ``nmx_proj`` (include/nmx.h): the layout's product on the GPU.  Stateless: one object may serve several plans
    with the same key list (the twins of other window lengths)."""

    def __init__(self, layout: ProjectionLayout, device: int = 0, lib=None) -> None:
        import ctypes as C

        from . import _lib
        from ._lib import get_library

        self.layout = layout
        self._lib = lib if lib is not None else get_library()
        self._h = C.c_void_p()
        self._arrays = [np.ascontiguousarray(a) for a in (layout.gather, layout.ptr, layout.idx, layout.w,
                                                           layout.out_col, layout.out_stride, layout.group_chan,
                                                           layout.point_group)]
        g, ptr, idx, w, oc, os_ = self._arrays[:6]
        d = _lib.ProjDesc()
        d.n_feat, d.n_chan, d.n_points = layout.n_feat, len(g), len(oc)
        i32, f64 = C.POINTER(C.c_int32), C.POINTER(C.c_double)
        d.gather, d.ptr, d.idx = g.ctypes.data_as(i32), ptr.ctypes.data_as(i32), idx.ctypes.data_as(i32)
        d.w = w.ctypes.data_as(f64)
        d.out_col, d.out_stride = oc.ctypes.data_as(i32), os_.ctypes.data_as(i32)
        d.n_groups = len(layout.group_chan) - 1
        d.group_chan, d.point_group = self._arrays[6].ctypes.data_as(i32), self._arrays[7].ctypes.data_as(i32)
        self._lib.check(self._lib.lib.nmx_proj_create(int(device), C.byref(d), C.byref(self._h)))

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                self._lib.lib.nmx_proj_destroy(h)
            except Exception:  # pragma: no cover - interpreter shutdown
                pass

    def process(self, rows: np.ndarray) -> np.ndarray:
        """In place on C-contiguous float32 host rows ``[n, >= n_keys + n_grid]``: the grid columns are written."""
        if rows.dtype != np.float32 or rows.ndim != 2 or not rows.flags.c_contiguous:
            raise ValueError("DeviceProjection.process needs C-contiguous float32 rows")
        self._lib.check(self._lib.lib.nmx_proj_process(self._h, rows.ctypes.data, rows.shape[1], rows.shape[0], 0, None))
        return rows

    def process_device(self, ptr: int, ld: int, n_rows: int, stream: int | None = None) -> None:
        """In place on device memory ``float32[n_rows][ld]`` (asynchronous on ``stream``)."""
        self._lib.check(self._lib.lib.nmx_proj_process(self._h, ptr, int(ld), int(n_rows), 1, stream))

    def process_table(self, table: np.ndarray) -> np.ndarray:
        """The float64 table ``[n, n_keys]`` (its values float32 numbers: the engine's rows, widened) -> the table widened
        by the grid columns, computed on the device."""
        lay = self.layout
        n = table.shape[0]
        wide = np.empty((n, lay.n_keys + lay.n_grid), np.float64)
        wide[:, :table.shape[1]] = table
        if n and lay.n_grid:
            rows = np.zeros((n, lay.n_keys + lay.n_grid), np.float32)
            rows[:, :lay.n_keys] = table[:, :lay.n_keys]
            self.process(rows)
            wide[:, lay.n_keys:] = rows[:, lay.n_keys:]
        return wide
