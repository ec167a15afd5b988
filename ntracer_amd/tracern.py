"""Mirror of the reference's ``ntracer.tracern`` module for the ray-cast path
(src/ntracer_body.hpp): BoxScene, CompositeScene, Camera, Vector, Matrix, AABB, the k-d node
and primitive value types and the lights.  Scenes own a handle of the HIP library; everything
else is a light fp32 value type used to describe a scene.

Scene construction (Triangle.from_points/to_points, prototypes, build_kdtree, build_composite_scene) lives in
``builder.py``: SURVEY section 8f item 1.  Not mirrored: pickling, TriangleBatchPointData-style introspection.
"""
import ctypes as C
import math
import os
import weakref

import numpy as np

from . import _lib, builder
from . import render as _render
from .render import Color, Material, Scene
from ._lib import NT_OUTLINE_SILHOUETTE, NT_OUTLINE_CREASE, NT_OUTLINE_DEPTH  # noqa: F401

BATCH_SIZE = _lib.NT_BATCH_SIZE     # tracer.hpp:34-38 (SSE reference build)
_ROUNDING_FUZZ = 1.1920928955078125e-07 * 10.0     # tracer.hpp:25
CUBE, SPHERE = 1, 2                  # wrapper.CUBE / wrapper.SPHERE (tracer.hpp:225)

f32 = np.float32


def _vec(n, values):
    if isinstance(values, Vector):
        if values.dimension != n:
            raise TypeError("vector has the wrong dimension")
        return values._v
    a = np.asarray(list(values), dtype=f32)
    if a.shape != (n,):
        raise TypeError("expected %d values" % n)
    return a


class Vector(_render.FloatBuffer):
    """tracern.Vector(dimension[,values]) -- fp32 n-vector (geometry.hpp:131-283).  memoryview(v) gives its floats."""
    __slots__ = ("_v",)

    def _float_buffer(self):
        a = self._v.view()
        a.flags.writeable = False
        return a

    def __init__(self, dimension, values=None):
        dimension = int(dimension)
        if dimension < 1:
            raise ValueError("dimension must be positive")
        self._v = np.zeros(dimension, f32) if values is None else _vec(dimension, values).copy()

    @classmethod
    def _wrap(cls, a):
        v = cls.__new__(cls)
        v._v = np.ascontiguousarray(a, dtype=f32)
        return v

    @staticmethod
    def axis(dimension, axis, length=1):
        v = np.zeros(int(dimension), f32)
        v[axis] = length
        return Vector._wrap(v)

    dimension = property(lambda s: len(s._v))

    def __reduce__(self):                               # obj_Vector_reduce, render.cpp:1705-1710
        return _render._vector_unpickle, (len(self._v), _render._encode_floats(self._v))

    def __len__(self):
        return len(self._v)

    def __getitem__(self, i):
        return float(self._v[i])

    def __iter__(self):
        return (float(x) for x in self._v)

    def __add__(self, o):
        return Vector._wrap(self._v + _vec(len(self._v), o))

    def __sub__(self, o):
        return Vector._wrap(self._v - _vec(len(self._v), o))

    def __neg__(self):
        return Vector._wrap(-self._v)

    def __mul__(self, s):
        return Vector._wrap(self._v * f32(s))

    __rmul__ = __mul__

    def __truediv__(self, s):
        return Vector._wrap(self._v / f32(s))

    def __eq__(self, o):
        try:
            return bool(np.array_equal(self._v, _vec(len(self._v), o)))
        except TypeError:
            return NotImplemented

    def __ne__(self, o):
        r = self.__eq__(o)
        return r if r is NotImplemented else not r

    def set_c(self, index, value):
        """Vector.set_c(index,value) -> a copy with one component replaced (ntracer_body.hpp:1998-2014)"""
        index = int(index)
        if index < 0 or index >= len(self._v):
            raise IndexError("vector index out of range")
        r = self._v.copy()
        r[index] = f32(value)
        return Vector._wrap(r)

    def square(self):
        return float(dot(self, self))

    def absolute(self):
        return float(np.sqrt(f32(dot(self, self))))

    def unit(self):
        return Vector._wrap(self._v / np.sqrt(f32(dot(self, self))))

    def apply(self, f):
        return Vector._wrap([f(float(x)) for x in self._v])

    def __repr__(self):
        return "Vector(%d,%r)" % (len(self._v), [float(x) for x in self._v])


def dot(a, b):
    """tracern.dot(a,b) -- fp32, summed left to right."""
    av = a._v if isinstance(a, Vector) else np.asarray(list(a), f32)
    bv = b._v if isinstance(b, Vector) else np.asarray(list(b), f32)
    if av.shape != bv.shape:
        raise TypeError("cannot perform dot product on vectors of different dimension")
    s = f32(av[0] * bv[0])
    for k in range(1, len(av)):
        s = f32(s + f32(av[k] * bv[k]))
    return float(s)


class Matrix(object):
    """tracern.Matrix(dimension,values) -- fp32 n x n (geometry.hpp:527-844); only what cameras and
    Solid orientations need."""
    __slots__ = ("_m",)

    def __init__(self, dimension, values):
        n = int(dimension)
        a = np.asarray([list(r) if not isinstance(r, (int, float)) else r for r in values], dtype=f32)
        if a.size != n * n:
            raise TypeError("expected %d values" % (n * n))
        self._m = a.reshape(n, n).copy()

    @classmethod
    def _wrap(cls, a):
        m = object.__new__(cls)
        m._m = np.ascontiguousarray(a, dtype=f32)
        return m

    dimension = property(lambda s: s._m.shape[0])

    def __reduce__(self):                               # obj_Matrix_reduce, render.cpp:1711-1715
        return _render._matrix_unpickle, (self._m.shape[0], _render._encode_floats(self._m.ravel()))

    @staticmethod
    def identity(dimension):
        return Matrix._wrap(np.eye(int(dimension), dtype=f32))

    @staticmethod
    def scale(dimension, s=None):
        n = int(dimension)
        if isinstance(s, (int, float)):
            return Matrix._wrap(np.eye(n, dtype=f32) * f32(s))
        return Matrix._wrap(np.diag(_vec(n, s)))

    @staticmethod
    def rotation(a, b, theta):
        """Matrix.rotation(a,b,theta): rotation_ (geometry.hpp:579-591), fp32."""
        av, bv = a._v, b._v
        n = len(av)
        c = f32(f32(math.cos(f32(theta))) - f32(1))
        s = f32(math.sin(f32(theta)))
        m = np.zeros((n, n), f32)
        for row in range(n):
            for col in range(n):
                x = f32(f32(av[row] * f32(f32(av[col] * c) - f32(bv[col] * s))) + f32(bv[row] * f32(f32(bv[col] * c) + f32(av[col] * s))))
                if col == row:
                    x = f32(x + f32(1))
                m[row, col] = x
        return Matrix._wrap(m)

    @staticmethod
    def reflection(a):
        """Matrix.reflection(a): I - 2 a a^T / |a|^2 (geometry.hpp:602-608), fp32."""
        av = a._v if isinstance(a, Vector) else np.asarray(list(a), f32)
        n = len(av)
        square = f32(dot(Vector._wrap(av), Vector._wrap(av)))
        m = np.zeros((n, n), f32)
        for row in range(n):
            for col in range(n):
                m[row, col] = f32(f32(1 if row == col else 0) - f32(f32(f32(f32(2) * av[row]) * av[col]) / square))
        return Matrix._wrap(m)

    def __getitem__(self, i):
        return Vector._wrap(self._m[i].copy())

    def __len__(self):
        return self._m.shape[0]

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    def determinant(self):
        """Matrix.determinant() (ntracer_body.hpp:2326-2330; the reference runs an fp32 LU, geometry.hpp:790-823)"""
        return float(f32(np.linalg.det(self._m.astype(np.float64))))

    @property
    def values(self):
        """all elements, row-major (an attribute in the reference: ntracer_body.hpp:2330-2345)"""
        return tuple(float(x) for x in self._m.ravel())

    def __mul__(self, o):
        if isinstance(o, Matrix):
            return Matrix._wrap(_matmul(self._m, o._m.T))
        if isinstance(o, Vector):
            return Vector._wrap([dot(Vector._wrap(r), o) for r in self._m])
        return NotImplemented

    def transpose(self):
        return Matrix._wrap(self._m.T.copy())

    def inverse(self):
        inv = np.linalg.inv(self._m.astype(np.float64))
        return Matrix._wrap(inv.astype(f32))

    def __eq__(self, o):
        return isinstance(o, Matrix) and bool(np.array_equal(self._m, o._m))

    def __repr__(self):
        return "Matrix(%d,%r)" % (len(self), list(self.values))


def _matmul(a, bt):
    """r[row][col] = dot(a[row], bt[col]) in fp32, left to right (geometry.hpp:556-575)."""
    n = a.shape[0]
    r = np.zeros((n, n), f32)
    for row in range(n):
        for col in range(n):
            r[row, col] = dot(Vector._wrap(a[row]), Vector._wrap(bt[col]))
    return r


class CameraAxes(object):
    def __init__(self, cam):
        self._cam = cam

    def __len__(self):
        return self._cam.dimension

    def __getitem__(self, i):
        return Vector._wrap(self._cam._axes[i].copy())

    def __setitem__(self, i, v):
        self._cam._axes[i] = _vec(self._cam.dimension, v)


class Camera(object):
    """tracern.Camera(dimension) -- camera.hpp:7-45: origin + orientation rows (right, up, forward, ...)."""

    def __init__(self, dimension):
        n = int(dimension)
        if n < 3:
            raise ValueError("dimension cannot be less than 3")
        self._origin = np.zeros(n, f32)
        self._axes = np.eye(n, dtype=f32)

    dimension = property(lambda s: len(s._origin))

    @property
    def origin(self):
        return Vector._wrap(self._origin.copy())

    @origin.setter
    def origin(self, v):
        self._origin = _vec(self.dimension, v).copy()

    @property
    def axes(self):
        return CameraAxes(self)

    def translate(self, v):
        """origin += v[i]*axes[i] (camera.hpp:17-19)."""
        v = _vec(self.dimension, v)
        for i in range(self.dimension):
            self._origin = self._origin + v[i] * self._axes[i]

    def transform(self, m):
        """t_orientation = t_orientation.mult_transpose(m) (camera.hpp:21-23)."""
        self._axes = _matmul(self._axes, m._m)

    def normalize(self):
        """Gram-Schmidt as camera.hpp:25-36 (fp32, same association order)."""
        n = self.dimension
        ax = self._axes
        new_axes = []
        for i in range(n - 1):
            x = np.zeros(n, f32)
            for j in range(i):
                x = x + f32(dot(Vector._wrap(ax[i + 1]), Vector._wrap(ax[j]))) * ax[j]
            new_axes.append(ax[i + 1] - x)
        out = np.zeros((n, n), f32)
        out[0] = ax[0] / np.sqrt(f32(dot(Vector._wrap(ax[0]), Vector._wrap(ax[0]))))
        for i in range(1, n):
            v = new_axes[i - 1]
            out[i] = v / np.sqrt(f32(dot(Vector._wrap(v), Vector._wrap(v))))
        self._axes = out

    def _copy(self):
        c = Camera(self.dimension)
        c._origin = self._origin.copy()
        c._axes = self._axes.copy()
        return c


class AABB(object):
    """tracern.AABB(dimension[,start,end]) -- tracer.hpp:1327-1356."""

    def __init__(self, dimension, start=None, end=None):
        n = int(dimension)
        self.dimension = n
        self.start = Vector(n, start) if start is not None else Vector._wrap(np.full(n, np.finfo(f32).min, f32))
        self.end = Vector(n, end) if end is not None else Vector._wrap(np.full(n, np.finfo(f32).max, f32))

    def __reduce__(self):                               # obj_AABB_reduce, render.cpp:1745-1752
        return _render._aabb_unpickle, (self.dimension, _render._encode_floats(np.concatenate([self.start._v, self.end._v])))

    def __eq__(self, o):
        if not isinstance(o, AABB):
            return NotImplemented
        return self.start == o.start and self.end == o.end

    def __ne__(self, o):
        r = self.__eq__(o)
        return r if r is NotImplemented else not r

    __hash__ = None

    def _check_axis(self, axis):
        axis = int(axis)
        if axis < 0 or axis >= self.dimension:
            raise IndexError("index out of range")
        return axis

    def left(self, axis, split):
        """AABB.left(axis,split): the part below the split (ntracer_body.hpp:2498-2513, tracer.hpp:1337-1343)."""
        axis = self._check_axis(axis)
        split = float(split)
        if not (self.start[axis] < split < self.end[axis]):
            raise ValueError("\"split\" must be inside the box within the given axis")
        e = self.end._v.copy()
        e[axis] = split
        return AABB(self.dimension, self.start._v, e)

    def right(self, axis, split):
        """AABB.right(axis,split): the part above the split."""
        axis = self._check_axis(axis)
        split = float(split)
        if not (self.start[axis] < split < self.end[axis]):
            raise ValueError("\"split\" must be inside the box within the given axis")
        b = self.start._v.copy()
        b[axis] = split
        return AABB(self.dimension, b, self.end._v)

    def intersects(self, primitive):
        """AABB.intersects(prototype) -> bool: whether the box and the primitive share a region of non-zero extent
        (two things that merely touch do not intersect; tracer.hpp:1459-1463).  The reference answers with
        projection tests (:1465-1700); here the primitive is clipped to the box exactly (nt_polytope_clip_box):
        a simplex as a polytope in its own plane, a cube solid as a parallelotope; a sphere solid by the distance
        from its centre to the box in the solid's own coordinates."""
        if not isinstance(primitive, PrimitivePrototype):
            raise TypeError("object is not an instance of PrimitivePrototype")
        if primitive.dimension != self.dimension:
            raise TypeError("cannot perform intersection test on object with different dimension")
        return primitive._overlaps(self.start._v.astype(np.float64), self.end._v.astype(np.float64))


class PointLight(object):
    """tracern.PointLight(position,color) -- tracer.hpp:1678-1689."""

    def __init__(self, position, color):
        self.position = position if isinstance(position, Vector) else Vector(len(list(position)), position)
        self.color = Color._coerce(color)

    dimension = property(lambda s: s.position.dimension)


class GlobalLight(object):
    """tracern.GlobalLight(direction,color) -- tracer.hpp:1691-1698."""

    def __init__(self, direction, color):
        self.direction = direction if isinstance(direction, Vector) else Vector(len(list(direction)), direction)
        self.color = Color._coerce(color)

    dimension = property(lambda s: s.direction.dimension)


# ---------------------------------------------------------------------------------------------
# primitives and k-d nodes: plain descriptions, flattened into nt_scene_desc by CompositeScene
# ---------------------------------------------------------------------------------------------
class Primitive(object):
    pass


class PrimitiveBatch(object):
    pass


class Triangle(Primitive):
    """tracern.Triangle(p1,face_normal,edge_normals,material) -- an (n-1)-simplex in plane /
    edge-normal form (tracer.hpp:392-488)."""

    def __init__(self, p1, face_normal, edge_normals, material):
        p1 = list(p1)
        n = len(p1)
        self.p1 = Vector(n, p1)
        self.face_normal = Vector(n, face_normal)
        self.edge_normals = tuple(Vector(n, e) for e in edge_normals)
        if len(self.edge_normals) != n - 1:
            raise ValueError("a simplex of dimension %d needs %d edge normals" % (n, n - 1))
        if not isinstance(material, Material):
            raise TypeError("material must be a Material")
        self.material = material
        self.d = -dot(self.face_normal, self.p1)       # recalculate_d (tracer.hpp:472-474)

    dimension = property(lambda s: s.p1.dimension)

    @staticmethod
    def from_points(points, material):
        """Triangle.from_points(points,material) -- tracer.hpp:442-462."""
        p1, fn, edges = builder.from_points_record([list(p) for p in points])
        return Triangle(p1, fn, edges, material)

    def to_points(self):
        """Triangle.to_points() -- tracer.hpp:490-506."""
        pts = builder.to_points_array(self.p1._v, self.face_normal._v, [e._v for e in self.edge_normals])
        return tuple(Vector._wrap(p) for p in pts)

    def _rows(self):
        return np.vstack([self.p1._v, self.face_normal._v] + [e._v for e in self.edge_normals])      # [n+1][n]

    def __eq__(self, o):
        if not isinstance(o, Triangle):
            return NotImplemented
        return self.dimension == o.dimension and np.array_equal(self._rows(), o._rows()) and self.material == o.material

    def __ne__(self, o):
        r = self.__eq__(o)
        return r if r is NotImplemented else not r

    __hash__ = object.__hash__

    def __reduce__(self):                               # obj_Triangle_reduce, ntracer_body.hpp:1217-1233
        return _render._triangle_unpickle, (self.dimension, _render._encode_floats(self._rows().ravel()), self.material)

    def _record(self):
        rec = [f32(self.d)] + list(self.face_normal._v) + list(self.p1._v)
        for e in self.edge_normals:
            rec += list(e._v)
        return np.asarray(rec, f32)


class TriangleBatch(PrimitiveBatch):
    """tracern.TriangleBatch(triangles): exactly BATCH_SIZE simplices (tracer.hpp:532-641)."""

    def __init__(self, triangles):
        tris = tuple(triangles)
        if len(tris) != BATCH_SIZE or not all(isinstance(t, Triangle) for t in tris):
            raise ValueError("exactly %d Triangle instances are required" % BATCH_SIZE)
        if len(set(t.dimension for t in tris)) != 1:
            raise TypeError("the triangles must have the same dimension")
        self._tris = tris

    dimension = property(lambda s: s._tris[0].dimension)

    def __len__(self):
        return BATCH_SIZE

    def __getitem__(self, i):
        return self._tris[i]

    def __reduce__(self):                               # rows [component][lane], render.cpp:1725-1735
        vals = np.stack([t._rows() for t in self._tris], axis=2)          # [n+1][n][BATCH_SIZE]
        return _render._triangle_batch_unpickle, (BATCH_SIZE, self.dimension, _render._encode_floats(vals.ravel())) + tuple(
            t.material for t in self._tris)


class Solid(Primitive):
    """tracern.Solid(type,position,orientation,material) -- tracer.hpp:231-289."""

    def __init__(self, type, position, orientation, material):
        if type not in (CUBE, SPHERE):
            raise ValueError("invalid shape type")
        if not isinstance(orientation, Matrix):
            raise TypeError("orientation must be a Matrix")
        n = orientation.dimension
        self.type = type
        self.orientation = orientation
        self.inv_orientation = orientation.inverse()
        self.position = Vector(n, position)
        if not isinstance(material, Material):
            raise TypeError("material must be a Material")
        self.material = material

    dimension = property(lambda s: s.orientation.dimension)

    def __reduce__(self):                               # obj_Solid_reduce, render.cpp:1736-1744
        data = bytes([self.type]) + _render._encode_floats(self.orientation._m.ravel()) + _render._encode_floats(self.position._v)
        return _render._solid_unpickle, (self.dimension, data, self.material)


class RayIntersection(object):
    """tracern.RayIntersection(dist,origin,normal,primitive,batch_index=-1) -- what KDNode.intersects / occludes answer
    with (ntracer_body.hpp:362-377, 1759-1810): the distance along the ray in units of |direction|, the normal ray of the
    surface (`origin`: the hit point, `normal`: its direction) and what was hit."""
    __slots__ = ("_dist", "_origin", "_normal", "_primitive", "_batch_index")

    def __init__(self, dist, origin, normal, primitive, batch_index=-1):
        batch_index = int(batch_index)
        if isinstance(primitive, Primitive):
            if batch_index != -1:
                raise ValueError('"batch_index" cannot be anything other than -1 unless "primitive" is an instance of PrimitiveBatch')
        elif isinstance(primitive, PrimitiveBatch):
            if batch_index < 0:
                raise ValueError('"batch_index" cannot be less than zero if "primitive" is an instance of PrimitiveBatch')
        else:
            raise TypeError('"primitive" must either be an instance of Primitive or PrimitiveBatch')
        origin = origin if isinstance(origin, Vector) else Vector(len(origin), origin)
        normal = normal if isinstance(normal, Vector) else Vector(len(normal), normal)
        if origin.dimension != normal.dimension:
            raise TypeError('"origin" and "normal" must have the same dimension')
        self._dist, self._origin, self._normal = float(dist), origin, normal
        self._primitive, self._batch_index = primitive, batch_index

    dist = property(lambda s: s._dist)
    origin = property(lambda s: s._origin)
    normal = property(lambda s: s._normal)
    primitive = property(lambda s: s._primitive)
    batch_index = property(lambda s: s._batch_index)

    def __repr__(self):
        return "RayIntersection(%r,%r,%r,%r,%r)" % (self._dist, self._origin, self._normal, self._primitive, self._batch_index)


class PrimaryHits(object):
    """What CompositeScene.primary_hits answers with: the primary-hit record of every pixel of a view, as numpy arrays or as
    torch tensors on the device, views of the buffers the library wrote -- dist, item, kind, index, lane, n_transparent
    [height][width] (with a camera table [count][height][width]) and, when asked for, normal_origin / normal_dir
    [...][n].  A pixel without an opaque hit has dist = FLT_MAX and item = kind = index = lane = -1."""

    def __init__(self, scene, width, height, frames, stride, hits, normal_origin, normal_dir):
        self._scene = scene
        self.width, self.height, self.frames = width, height, frames
        self.hits = hits                                  # the raw records: [frames * stride][4] int32 (dist's bits, item, lane, n_transparent)

        def shaped(a):                                    # [frames * stride][k] -> [frames][height][width][k], or [height][width][k]
            if a is None:
                return None
            k = a.shape[-1]
            a = a.reshape(frames or 1, stride, k)[:, :width * height].reshape(frames or 1, height, width, k)
            return a if frames is not None else a[0]
        h = shaped(hits)
        self.dist = _as_f32(h[..., 0])
        self.item, self.lane, self.n_transparent = h[..., 1], h[..., 2], h[..., 3]
        self.normal_origin, self.normal_dir = shaped(normal_origin), shaped(normal_dir)

    @property
    def kind(self):
        return (self.item & 3) - 4 * _as_i32(self.item < 0)

    @property
    def index(self):
        miss = _as_i32(self.item < 0)
        return (self.item >> 2) * (1 - miss) - miss

    def intersection(self, x, y, frame=0):
        """the RayIntersection under pixel (x, y), its `primitive` the scene's own object, or None where the ray hits nothing
        opaque; needs the normals (primary_hits(..., normals=True))"""
        at = (int(y), int(x)) if self.frames is None else (int(frame), int(y), int(x))
        item = int(self.item[at])
        if item < 0:
            return None
        if self.normal_origin is None:
            raise ValueError("intersection() needs the normal rays: ask for them with primary_hits(..., normals=True)")
        host = lambda a: np.asarray(a.cpu() if hasattr(a, "cpu") else a, f32).copy()
        return RayIntersection(float(self.dist[at]), Vector._wrap(host(self.normal_origin[at])), Vector._wrap(host(self.normal_dir[at])),
                               self._scene._object_of(item & 3, item >> 2), int(self.lane[at]))


class FaceHits(object):
    """What BoxScene.face_hits answers with: which face of the cube every pixel of a view sees and how far away it is, as numpy
    arrays or as torch tensors on the device, views of the records the library wrote -- dist (FLT_MAX: nothing), axis (the axis
    the face is perpendicular to, -1: nothing), side (1: the face at +1, 0: the face at -1, -1: nothing) and hit (bool), each
    [height][width], with a camera table [count][height][width]; records is the raw buffer, [frames * stride][4] int32 (dist's
    bits, axis, side, 0)."""

    def __init__(self, dimension, width, height, frames, stride, records):
        self.dimension = dimension
        self.width, self.height, self.frames = width, height, frames
        self.records = records
        r = records.reshape(frames or 1, stride, 4)[:, :width * height].reshape(frames or 1, height, width, 4)
        if frames is None:
            r = r[0]
        self.dist = _as_f32(r[..., 0])
        self.axis, self.side = r[..., 1], r[..., 2]
        self.hit = self.axis >= 0

    def normal(self, x, y, frame=0):
        """the outward unit normal of the face under pixel (x, y) as a Vector, or None where the ray sees nothing"""
        at = (int(y), int(x)) if self.frames is None else (int(frame), int(y), int(x))
        axis = int(self.axis[at])
        if axis < 0:
            return None
        return Vector.axis(self.dimension, axis, 1.0 if int(self.side[at]) else -1.0)


class HitLayers(object):
    """What CompositeScene.hit_layers answers with: the `layers` nearest surfaces under every pixel of a view, nearest first
    (include/ntracer_hip.h has the rule), as numpy arrays or as torch tensors on the device, views of the records the library
    wrote.  records is the raw buffer, int32 [layers][height][width][4] (dist's bits, item, lane, count); dist (FLT_MAX: no such
    layer), item, kind, index and lane (-1: no such layer) are [layers][height][width]; count [height][width] is the pixel's
    full crossing count -- crossing_counts' number -- and cut says where it exceeds `layers`, so that the list was cut."""

    def __init__(self, scene, width, height, layers, records):
        self._scene = scene
        self.width, self.height, self.layers = width, height, layers
        self.records = records
        self.dist = _as_f32(records[..., 0])
        self.item, self.lane = records[..., 1], records[..., 2]
        self.count = records[0, :, :, 3]
        self.cut = self.count > layers

    kind = PrimaryHits.kind
    index = PrimaryHits.index

    def primitive(self, x, y, layer=0):
        """(the scene's own object, batch_index) of layer `layer` under pixel (x, y) -- batch_index is the simplex inside a
        TriangleBatch, -1 otherwise -- or None where the pixel has no such layer"""
        at = (int(layer), int(y), int(x))
        item = int(self.item[at])
        if item < 0:
            return None
        return self._scene._object_of(item & 3, item >> 2), int(self.lane[at])


def _as_f32(a):
    """the same 32 bits as fp32: numpy or torch"""
    if hasattr(a, "is_cuda"):
        import torch
        return a.view(torch.float32)
    return a.view(f32)


def _as_i32(a):
    if hasattr(a, "is_cuda"):
        import torch
        return a.to(torch.int32)
    return a.astype(np.int32)


class KDNode(object):
    """tracern.KDNode: base of KDLeaf / KDBranch.  The two ray queries of the reference (ntracer_body.hpp:1412-1496) run
    on the device, one ray a call here -- CompositeScene.intersect_rays / occludes_rays are the batched forms underneath."""
    _owner = None           # weak reference to the CompositeScene this node is the root of
    _private = None         # ... or a scene of its own, made on first use (its boundary is never consulted by a query)

    def _query_scene(self):
        sc = self._owner() if self._owner is not None else None
        if sc is None:
            if self._private is None:
                n = self.dimension
                self._private = CompositeScene._for_node(AABB(n, [-1.0] * n, [1.0] * n), self)
            sc = self._private
        return sc

    def _ray_args(self, origin, direction, source, batch_index):
        o = origin if isinstance(origin, Vector) else Vector(len(origin), origin)
        d = direction if isinstance(direction, Vector) else Vector(len(direction), direction)
        if o.dimension != d.dimension:
            raise TypeError('"origin" and "direction" must have the same dimension')
        if o.dimension != self.dimension:
            raise TypeError("the ray and the node must have the same dimension")
        if source is not None and not isinstance(source, (Primitive, PrimitiveBatch)):
            raise TypeError('"source" must be an instance of Primitive or PrimitiveBatch')
        sc = self._query_scene()
        item = sc._item_of(source) if source is not None else -1
        lane = int(batch_index) if isinstance(source, PrimitiveBatch) else -1
        return sc, o._v[None], d._v[None], np.asarray([item], np.int32), np.asarray([lane], np.int32)

    def intersects(self, origin, direction, t_near=None, t_far=None, source=None, batch_index=-1):
        """KDNode.intersects(origin,direction,t_near,t_far,source,batch_index): the transparent hits, then the opaque hit
        if there is one, as RayIntersection objects."""
        sc, o, d, si, sl = self._ray_args(origin, direction, source, batch_index)
        r = sc.intersect_rays(o, d, None if t_near is None else [t_near], None if t_far is None else [t_far], si, sl,
                              normals=True, max_transparent=_lib.NT_TH_MAX)
        hits = sc._transparent_hits(o[0], d[0], r["transparent"][0], int(r["n_transparent"][0]))
        if r["kind"][0] >= 0:
            hits.append(RayIntersection(float(r["dist"][0]), Vector._wrap(r["normal_origin"][0].copy()), Vector._wrap(r["normal"][0].copy()),
                                        sc._object_of(int(r["kind"][0]), int(r["index"][0])), int(r["lane"][0])))
        return hits

    def occludes(self, origin, direction, distance=None, t_near=None, t_far=None, source=None, batch_index=-1):
        """KDNode.occludes(origin,direction,distance,t_near,t_far,source,batch_index): (occluded, hits) -- the transparent
        hits met on the way when nothing opaque lies nearer than `distance`, else None."""
        sc, o, d, si, sl = self._ray_args(origin, direction, source, batch_index)
        r = sc.occludes_rays(o, d, None if distance is None else [distance], None if t_near is None else [t_near],
                             None if t_far is None else [t_far], si, sl, max_transparent=_lib.NT_TH_MAX)
        if r["blocked"][0]:
            return True, None
        return False, sc._transparent_hits(o[0], d[0], r["transparent"][0], int(r["n_transparent"][0]))


class KDLeaf(KDNode):
    """tracern.KDLeaf(primitives): batches are kept in front (tracer.hpp:1146-1150)."""

    def __init__(self, primitives):
        prims = list(primitives)
        if not prims:
            raise ValueError("KDLeaf requires at least one item")
        for p in prims:
            if not isinstance(p, (Primitive, PrimitiveBatch)):
                raise TypeError("object is not an instance of Primitive or PrimitiveBatch")
        if len(set(p.dimension for p in prims)) != 1:
            raise TypeError("every member of KDLeaf must have the same dimension")
        self._items = tuple([p for p in prims if isinstance(p, PrimitiveBatch)] +
                            [p for p in prims if not isinstance(p, PrimitiveBatch)])

    dimension = property(lambda s: s._items[0].dimension)

    def __len__(self):
        return len(self._items)

    def __getitem__(self, i):
        return self._items[i]


class KDBranch(KDNode):
    """tracern.KDBranch(axis,split[,left=None,right=None]) -- tracer.hpp:813-830."""

    def __init__(self, axis, split, left=None, right=None):
        if left is None and right is None:
            raise ValueError('"left" and "right" can\'t both be None')
        for c in (left, right):
            if c is not None and not isinstance(c, KDNode):
                raise TypeError("child is not a KDNode")
        if left is not None and right is not None and left.dimension != right.dimension:
            raise TypeError("the nodes must have the same dimension")
        self.axis = int(axis)
        self.split = float(f32(split))
        self.left = left
        self.right = right
        if self.axis < 0 or self.axis >= self.dimension:
            raise ValueError("invalid axis")

    dimension = property(lambda s: (s.left if s.left is not None else s.right).dimension)


class Lens(object):
    """Lens(width, height, coeffs) -- a projection that keeps the eye in one point, as a table of [height][width][3] float32
    coefficients (sx, sy, sz): pixel (x, y)'s ray leaves the camera along (forward * sz + right * sx) - up * sy, normalised
    as the pinhole's ray is (include/ntracer_hip.h).  An entry that is all zero, or holds a NaN, is a masked pixel: no ray,
    colour (0, 0, 0).  Set on a scene (Scene.set_lens) it replaces the pinhole of every render; the table does not depend on
    the camera and is uploaded once a device.  The constructors compute in float64 and round once, with u = x - width / 2 and
    v = y - height / 2 -- the pinhole's own pixel coordinates."""

    def __init__(self, width, height, coeffs):
        for v in (width, height):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError("the size of a lens must be two integers")
        width, height = int(width), int(height)
        if width < 1 or height < 1:
            raise ValueError("the size of a lens must be positive")
        c = np.ascontiguousarray(coeffs, f32)
        if c.shape != (height, width, 3):
            raise ValueError("coeffs must have shape (%d, %d, 3)" % (height, width))
        self._handle = None
        h = _lib.lib().nt_lens_create(width, height, c.ctypes.data_as(_lib.f32p))
        if not h:
            raise ValueError(_lib.last_error())
        self._handle = h

    @classmethod
    def _adopt(cls, handle):
        if not handle:
            raise ValueError(_lib.last_error())
        self = cls.__new__(cls)
        self._handle = handle
        return self

    def __del__(self):
        h, self._handle = getattr(self, "_handle", None), None
        if h:
            try:
                _lib.lib().nt_lens_destroy(h)
            except Exception:
                pass

    width = property(lambda s: int(_lib.lib().nt_lens_width(s._handle)))
    height = property(lambda s: int(_lib.lib().nt_lens_height(s._handle)))

    @property
    def coeffs(self):
        """the float32 table, [height][width][3] (a copy)"""
        out = np.zeros((self.height, self.width, 3), f32)
        _lib.check(_lib.lib().nt_lens_coeffs(self._handle, out.ctypes.data_as(_lib.f32p)))
        return out

    @property
    def masked(self):
        """[height][width] bool: the pixels that cast no ray"""
        c = self.coeffs
        return np.isnan(c).any(axis=2) | (c == 0).all(axis=2)

    @staticmethod
    def _grid(width, height):
        width, height = int(width), int(height)
        if width < 1 or height < 1:
            raise ValueError("the size of a lens must be positive")
        u = np.arange(width, dtype=np.float64)[None, :] - width / 2.0
        v = np.arange(height, dtype=np.float64)[:, None] - height / 2.0
        return width, height, np.broadcast_to(u, (height, width)), np.broadcast_to(v, (height, width))

    @classmethod
    def pinhole(cls, width, height, fov):
        """the flat pinhole of a scene with this fov, built by the library from the ray source's own expressions: a render
        through it is the plain render, bit for bit"""
        return cls._adopt(_lib.lib().nt_lens_create_pinhole(int(width), int(height), float(fov)))

    @classmethod
    def fisheye(cls, width, height, fov):
        """equidistant fisheye: the angle from the axis grows linearly with the distance from the centre, fov / 2 at the
        distance width / 2; fov up to 2 pi; pixels beyond the angle pi are masked"""
        fov = float(fov)
        if not (0.0 < fov <= 2.0 * math.pi):
            raise ValueError("the fov of a fisheye must be in (0, 2 pi]")
        width, height, u, v = cls._grid(width, height)
        r = np.hypot(u, v)
        theta = r * (fov / 2.0) / (width / 2.0)
        rs = np.where(r == 0.0, 1.0, r)
        c = np.stack([np.sin(theta) * u / rs, np.sin(theta) * v / rs, np.cos(theta)], axis=2)
        c[r == 0.0] = (0.0, 0.0, 1.0)
        c[theta > math.pi] = 0.0
        return cls(width, height, c.astype(f32))

    @classmethod
    def equirectangular(cls, width, height, hfov=2.0 * math.pi, vfov=math.pi):
        """longitude across, latitude down: the full sphere by default"""
        width, height, u, v = cls._grid(width, height)
        lam = u * float(hfov) / width
        phi = v * float(vfov) / height
        c = np.stack([np.sin(lam) * np.cos(phi), np.sin(phi), np.cos(lam) * np.cos(phi)], axis=2)
        return cls(width, height, c.astype(f32))

    @classmethod
    def cylindrical(cls, width, height, hfov):
        """longitude across, a flat projection down (the scale of the axis' pixel)"""
        width, height, u, v = cls._grid(width, height)
        lam = u * float(hfov) / width
        c = np.stack([np.sin(lam), v * float(hfov) / width, np.cos(lam)], axis=2)
        return cls(width, height, c.astype(f32))

    def directions(self, camera):
        """The unnormalised direction of every pixel's ray for `camera`, float32 [height * width][n], computed in float32 in
        the device's operation order; zero rows for masked pixels.  With them Scene.render_rays / ray_colors /
        intersect_rays reproduce what a render through the lens casts."""
        if not isinstance(camera, Camera):
            raise TypeError("camera must be a Camera")
        c = self.coeffs.reshape(-1, 3)
        ax = np.ascontiguousarray(camera._axes, f32)
        right, up, fwd = ax[0][None, :], ax[1][None, :], ax[2][None, :]
        sx, sy, sz = c[:, 0:1], c[:, 1:2], c[:, 2:3]
        with np.errstate(invalid="ignore"):
            v = (fwd * sz + right * sx) - up * sy
        v[self.masked.reshape(-1)] = 0
        return np.ascontiguousarray(v, f32)


def clip_plane_through(point, normal):
    """The (normal, offset) pair of set_clip_planes for the plane through `point` with the given normal, which keeps the side
    the normal points away from: the normal's components as float32, the offset their float64 dot product with the point
    rounded once to float32."""
    a = np.asarray([float(v) for v in normal], f32)
    p = np.asarray([float(v) for v in point], np.float64)
    if a.shape != p.shape or a.ndim != 1:
        raise ValueError("point and normal must have the same number of components")
    return tuple(float(v) for v in a), float(f32(np.dot(a.astype(np.float64), p)))


def sphere_directions(n, count, seed=0):
    """`count` directions uniform on the unit sphere of n dimensions, float32 [count][n]: normal deviates of
    numpy.random.default_rng(seed), normalised in float64 -- the table set_ambient_occlusion makes of a plain sample count"""
    n, count = int(n), int(count)
    if n < 1 or count < 0:
        raise ValueError("sphere_directions wants a positive dimension and a count that is not negative")
    v = np.random.default_rng(seed).standard_normal((count, n))
    return np.ascontiguousarray(v / np.sqrt((v * v).sum(axis=1))[:, None], f32)


def aperture_disc(n, K, radius):
    """(offsets float32 [K][n], weights float32 [K][3]) for set_view_stack: a lens of the given radius in the camera's right/up
    plane -- sample 0 at the centre, samples 1 .. K - 1 a sunflower (radius * sqrt(k / (K - 1)), the golden angle apart), the
    same table every time -- and weights 1 / K each.  Use it with a focus: depth of field."""
    n, K = int(n), int(K)
    if n < 3 or K < 1 or K > _lib.NT_STACK_MAX or not float(radius) >= 0.0:
        raise ValueError("aperture_disc wants n >= 3, 1 <= K <= %d and a radius that is not negative" % _lib.NT_STACK_MAX)
    off = np.zeros((K, n), f32)
    golden = math.pi * (3.0 - math.sqrt(5.0))
    for k in range(1, K):
        r = float(radius) * math.sqrt(k / float(K - 1))
        off[k, 0] = r * math.cos(k * golden)
        off[k, 1] = r * math.sin(k * golden)
    return off, np.full((K, 3), f32(1) / f32(K), f32)


def slab(n, axis, half_thickness, K, colors=None):
    """(offsets float32 [K][n], weights float32 [K][3]) for set_view_stack: K evenly spaced offsets from -half_thickness to
    +half_thickness along the hidden axis `axis` >= 3 of the camera (K = 1: the slice itself), no focus.  colors None: weights
    1 / K each, the projection view of the slab.  colors = (lo, mid, hi), three (r, g, b): an onion skin -- a sample's weight
    is the colour interpolated from lo at -half_thickness over mid at 0 to hi at +half_thickness, divided by K."""
    n, K, axis = int(n), int(K), int(axis)
    if n < 4 or not 3 <= axis < n or K < 1 or K > _lib.NT_STACK_MAX or not float(half_thickness) >= 0.0:
        raise ValueError("slab wants a hidden axis (3 <= axis < n), 1 <= K <= %d and a half_thickness that is not negative" % _lib.NT_STACK_MAX)
    t = np.linspace(-1.0, 1.0, K) if K > 1 else np.zeros(1)
    off = np.zeros((K, n), f32)
    off[:, axis] = t * float(half_thickness)
    if colors is None:
        return off, np.full((K, 3), f32(1) / f32(K), f32)
    lo, mid, hi = (np.asarray(c, np.float64).reshape(3) for c in colors)
    w = np.where(t[:, None] < 0.0, mid + (lo - mid) * (-t[:, None]), mid + (hi - mid) * t[:, None]) / float(K)
    return off, np.ascontiguousarray(w, f32)


def stereo_pair(n, separation):
    """(offsets float32 [2][n], weights float32 [2][3]) for set_view_stack: the left eye -separation / 2 and the right eye
    +separation / 2 along the camera's right axis, the left in red and the right in cyan.  Use it with a focus, the distance at
    which the two pictures coincide: an anaglyph."""
    n = int(n)
    if n < 3:
        raise ValueError("stereo_pair wants n >= 3")
    off = np.zeros((2, n), f32)
    off[0, 0] = -float(separation) / 2.0
    off[1, 0] = float(separation) / 2.0
    return off, np.asarray([[1, 0, 0], [0, 1, 1]], f32)


class _SceneBase(Scene):
    """Camera / fov handling shared by BoxScene and CompositeScene (ntracer_body.hpp:676-715)."""

    def _init_common(self, n):
        self._n = n

    dimension = property(lambda s: s._n)

    @property
    def fov(self):
        return float(_lib.lib().nt_scene_get_fov(self._handle))

    def set_fov(self, fov):
        _lib.check(_lib.lib().nt_scene_set_fov(self._handle, float(fov)))

    @property
    def supersampling(self):
        """s: every pixel is the mean of s x s rays (1: one ray a pixel, the reference's only mode)"""
        return int(_lib.lib().nt_scene_get_supersampling(self._handle))

    def set_supersampling(self, factor):
        """Render with factor x factor samples a pixel (1..8), box-filtered on the device: the s*W x s*H frame of the same view,
        each sample's colour clamped to [0, 1], averaged in fp32 and packed as always.  A view setting like
        fov: not pickled.  Probes (calculate_color, colors_at) answer for one ray."""
        if isinstance(factor, bool) or not isinstance(factor, (int, np.integer)):
            raise ValueError("the supersampling factor must be an integer between 1 and 8")
        _lib.check(_lib.lib().nt_scene_set_supersampling(self._handle, int(factor)))

    @property
    def supersampling_scratch_mb(self):
        """cap of the device buffer that holds the samples, MiB per device (default 1024)"""
        return int(_lib.lib().nt_scene_get_supersampling_scratch_mb(self._handle))

    def set_supersampling_scratch_mb(self, mib):
        """A supersampled job whose samples (12 * s * s bytes a pixel) exceed the cap is rendered in chunks of frames and,
        below one frame, of rows -- same pixels; the samples of one row must fit."""
        if isinstance(mib, bool) or not isinstance(mib, (int, np.integer)):
            raise ValueError("the supersampling scratch cap must be an integer number of MiB")
        _lib.check(_lib.lib().nt_scene_set_supersampling_scratch_mb(self._handle, int(mib)))

    @property
    def adaptive_supersampling(self):
        """None, or the contrast threshold above which a pixel gets the s x s samples (set_adaptive_supersampling)"""
        on, t = C.c_int(0), C.c_float(0.0)
        _lib.check(_lib.lib().nt_scene_get_adaptive_supersampling(self._handle, C.byref(on), C.byref(t)))
        return float(t.value) if on.value else None

    def set_adaptive_supersampling(self, threshold):
        """With a supersampling factor above 1, refine only the pixels that show contrast: a pixel whose plain single-sample
        colour (clamped to [0, 1]) differs from that of one of its four neighbours by more than `threshold` in some component
        gets the factor's s x s samples, every other pixel keeps the plain colour.  None takes it off; a
        negative threshold refines every pixel, 1 or more refines none.  A feature thinner than a pixel that every pixel-centre
        ray misses is not seen.  Row bands and statistics are refused with it.  A view setting like fov: not pickled."""
        if threshold is None:
            _lib.check(_lib.lib().nt_scene_set_adaptive_supersampling(self._handle, 0, 0.0))
            return
        if isinstance(threshold, bool) or not isinstance(threshold, (int, float, np.integer, np.floating)):
            raise ValueError("the adaptive threshold must be a finite number or None")
        _lib.check(_lib.lib().nt_scene_set_adaptive_supersampling(self._handle, 1, float(threshold)))

    def refinement_mask(self, width, height, device=None, strict_reference=None):
        """The pixels a width x height render of the scene's camera would refine under the adaptive threshold that is set
        (nt_adaptive_mask), whatever the factor: a numpy bool array [height][width] -- or, with `device` a torch device, a
        torch bool tensor there, enqueued on torch's current stream."""
        mask = self._view_query("nt_adaptive_mask", width, height, device, np.uint8, "adaptive_supersampling",
                                "the adaptive threshold is off (set_adaptive_supersampling)", strict_reference, counted=True, zeroed=True)
        if device is None:
            return mask.view(np.bool_)
        import torch
        return mask.view(torch.bool)

    def _view_query(self, entry, width, height, device, dtype, setting, off_message, strict_reference=None, tail=(), counted=False,
                    zeroed=False, plain=False):
        """What refinement_mask, occlusion_counts, outline_mask, depth_cue_factors and face_line_mask share: the buffer of `entry`
        (include/ntracer_hip.h) for a width x height view, `dtype` [height][width] + tail -- a numpy array through the host form,
        or with `device` a torch device a tensor there (zeroed first, or as allocated) through the _device form on torch's current
        stream.  `setting` is the property that is None while the setting is off, which the device path says in `off_message` (None: no setting is needed).
        `counted`: the host form takes a pointer for a count as well, not asked for.  `plain`: an entry without
        strict_reference, whose options carry the device alone, and whose "off" answer needs no torch."""
        width, height = int(width), int(height)
        if width < 1 or height < 1:
            raise ValueError("the size of a view must be positive")
        L = _lib.lib()
        shape = (height, width) + tuple(tail)
        if device is None:
            opts = _lib.NtRenderOpts()
            opts.device = -1
            if not plain:
                if strict_reference is None:
                    strict_reference = os.environ.get("NTRACER_STRICT_REFERENCE", "0") not in ("", "0")
                opts.strict_reference = 1 if strict_reference else 0
            out = np.zeros(shape, dtype)
            _lib.check(getattr(L, entry)(self._handle, width, height, out.ctypes.data, *((None,) if counted else ()), C.byref(opts)))
            return out
        if plain and setting is not None and getattr(self, setting) is None:
            raise ValueError(off_message)
        import torch
        dev = torch.device(device)
        if dev.type != "cuda":
            raise ValueError("device must be a HIP device")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if not plain and setting is not None and getattr(self, setting) is None:
            raise ValueError(off_message)
        out = (torch.zeros if zeroed else torch.empty)(shape, dtype=getattr(torch, np.dtype(dtype).name), device=dev)
        if plain:
            opts = _lib.NtRenderOpts()
            opts.device = dev.index
        else:
            opts = self._rays_opts(dev, strict_reference)
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(getattr(L, entry + "_device")(self._handle, width, height, C.c_void_p(out.data_ptr()), C.byref(opts), C.c_void_p(stream)))
        return out

    def set_ambient_occlusion(self, samples, radius=None, bias=None, strength=1.0):
        """Darken every pixel of a render by how enclosed its primary hit is (include/ntracer_hip.h): of K short
        rays cast from the hit point into the hemisphere of the side the primary ray came from, `blocked` find an opaque
        surface within `radius`, and the pixel's plain colour is multiplied by 1 - strength * blocked / K.  `samples`: an int K
        (1..256), meaning sphere_directions(n, K); or a [K][n] array of directions, used as given (the radius is in units of
        their length); or None / 0 for off, which needs no radius.  `bias` lifts the rays' origin off the surface along its normal (None:
        1e-3 * radius).  CompositeScene only.  Supersampling, row bands, statistics, a lens and the parallel projection are
        refused with it; calculate_color / colors_at, primary_hits, ray_colors, render_rays and the ray queries ignore it.  A
        view setting like fov: not pickled."""
        L = _lib.lib()
        if samples is None or (isinstance(samples, (int, np.integer)) and not isinstance(samples, bool) and int(samples) == 0):
            _lib.check(L.nt_scene_set_ambient_occlusion(self._handle, 0, None, 0.0, 0.0, 0.0))
            return
        if isinstance(samples, bool):
            raise ValueError("samples must be a count, an array of directions or None")
        if radius is None:
            raise ValueError("ambient occlusion wants a radius")
        for v in (radius, strength) + (() if bias is None else (bias,)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
                raise ValueError("radius, bias and strength must be numbers")
        if isinstance(samples, (int, np.integer)):
            if int(samples) < 0:
                raise ValueError("the number of ambient occlusion samples must be between 0 and 256")
            table = sphere_directions(self._n, int(samples))
        else:
            table = np.ascontiguousarray(samples, f32)
            if table.ndim != 2 or table.shape[1] != self._n:
                raise ValueError("the directions must be a [K][%d] array" % self._n)
        if bias is None:
            bias = 1e-3 * float(radius)
        _lib.check(L.nt_scene_set_ambient_occlusion(self._handle, len(table), table.ctypes.data_as(_lib.f32p), float(radius), float(bias),
                                                    float(strength)))

    @property
    def ambient_occlusion(self):
        """None, or a dict of the setting: count, directions (float32 [count][n]), radius, bias, strength"""
        L = _lib.lib()
        count, radius, bias, strength = C.c_int(0), C.c_float(0.0), C.c_float(0.0), C.c_float(0.0)
        _lib.check(L.nt_scene_get_ambient_occlusion(self._handle, C.byref(count), None, C.byref(radius), C.byref(bias), C.byref(strength)))
        if count.value <= 0:
            return None
        table = np.zeros((count.value, self._n), f32)
        _lib.check(L.nt_scene_get_ambient_occlusion(self._handle, None, table.ctypes.data_as(_lib.f32p), None, None, None))
        return dict(count=int(count.value), directions=table, radius=float(radius.value), bias=float(bias.value), strength=float(strength.value))

    def occlusion_counts(self, width, height, device=None, strict_reference=None):
        """The blocked counts of a width x height view of the scene's camera under the ambient occlusion that is set
        (nt_ambient_occlusion): int32 [height][width], -1 where the primary ray finds nothing opaque, else how many of the K
        samples are blocked -- a numpy array, or with `device` a torch device a torch tensor there, enqueued on torch's
        current stream."""
        return self._view_query("nt_ambient_occlusion", width, height, device, np.int32, "ambient_occlusion",
                                "ambient occlusion is off (set_ambient_occlusion)", strict_reference)

    def set_outlines(self, crease_angle=0.1, depth_gap=0.02, color=(0, 0, 0), strength=1.0):
        """Draw a line along the silhouette, along every edge where two facets meet and along every jump in depth (DESIGN.md
        4.11, include/ntracer_hip.h), from the primary hits of the render itself.  A pixel with an opaque hit is marked when one
        of its four neighbours hits nothing, or hits another simplex no nearer than the pixel's own whose normal makes more than
        `crease_angle` (radians, up to sign; crease_cos = float32(cos(angle))) with the pixel's, or which lies farther by more
        than `depth_gap` times the pixel's distance (0: no depth lines); a marked pixel's plain colour P becomes
        P * (1 - strength) + color * strength.  set_outlines(None) takes the setting off.  CompositeScene only.  Supersampling,
        row bands, statistics, a lens, the parallel projection and ambient occlusion are refused with it; calculate_color /
        colors_at, primary_hits, ray_colors, render_rays, the ray queries, refinement_mask and occlusion_counts ignore it.  A
        view setting like fov: not pickled."""
        L = _lib.lib()
        if crease_angle is None:
            _lib.check(L.nt_scene_set_outlines(self._handle, 0, 0.0, 0.0, None, 0.0))
            return
        for v in (crease_angle, depth_gap, strength):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
                raise ValueError("crease_angle, depth_gap and strength must be numbers")
        col = np.ascontiguousarray([float(c) for c in color], f32)
        if col.shape != (3,):
            raise ValueError("color must have three components")
        if not 0.0 <= float(crease_angle) <= math.pi / 2:
            raise ValueError("crease_angle must lie between 0 and pi / 2 radians")
        crease_cos = f32(math.cos(float(crease_angle)))
        _lib.check(L.nt_scene_set_outlines(self._handle, 1, float(crease_cos), float(depth_gap), col.ctypes.data_as(_lib.f32p), float(strength)))

    @property
    def outlines(self):
        """None, or a dict of the setting: crease_cos, depth_gap, color (three floats), strength"""
        on, cc, gap, st = C.c_int(0), C.c_float(0.0), C.c_float(0.0), C.c_float(0.0)
        col = np.zeros(3, f32)
        _lib.check(_lib.lib().nt_scene_get_outlines(self._handle, C.byref(on), C.byref(cc), C.byref(gap), col.ctypes.data_as(_lib.f32p), C.byref(st)))
        if not on.value:
            return None
        return dict(crease_cos=float(cc.value), depth_gap=float(gap.value), color=tuple(float(c) for c in col), strength=float(st.value))

    def outline_mask(self, width, height, device=None, strict_reference=None):
        """The outline mask of a width x height view of the scene's camera under the setting that is on (nt_outline_mask): uint8
        [height][width], 0 or an OR of NT_OUTLINE_SILHOUETTE, NT_OUTLINE_CREASE and NT_OUTLINE_DEPTH -- a numpy array, or with
        `device` a torch device a torch tensor there, enqueued on torch's current stream."""
        return self._view_query("nt_outline_mask", width, height, device, np.uint8, "outlines", "outlines are off (set_outlines)",
                                strict_reference, counted=True)

    def set_xray(self, absorbance=0.2, tint=1.0):
        """Draw the inside (include/ntracer_hip.h): every primitive the primary ray of a pixel crosses -- all of
        them, in no order, with no cap -- multiplies the background behind it by its material's transmittance
        T = clamp01(1 - absorbance * (1 - tint * color)) per channel.  tint = 0 is the grey X-ray, (1 - absorbance) ** count;
        tint = 1 is stained glass.  Opacity, lights, shadows and reflections play no part.  set_xray(None) takes the setting off.
        CompositeScene only.  Supersampling, row bands, statistics, a lens, the parallel projection, a view stack, clip planes,
        depth cues, outlines and ambient occlusion are refused with it, and so are calculate_color / colors_at, ray_colors,
        render_rays, refinement_mask, occlusion_counts, outline_mask and depth_cue_factors while it is on; primary_hits and the
        ray queries ignore it.  A view setting like fov: not pickled."""
        L = _lib.lib()
        if absorbance is None:
            _lib.check(L.nt_scene_set_xray(self._handle, 0, 0.0, 0.0))
            return
        for v in (absorbance, tint):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
                raise ValueError("absorbance and tint must be numbers")
        _lib.check(L.nt_scene_set_xray(self._handle, 1, float(absorbance), float(tint)))

    @property
    def xray(self):
        """None, or a dict of the setting: absorbance, tint, transmittance (float32 [n_materials][3], the table the kernels read)"""
        L = _lib.lib()
        on, ab, ti = C.c_int(0), C.c_float(0.0), C.c_float(0.0)
        _lib.check(L.nt_scene_get_xray(self._handle, C.byref(on), C.byref(ab), C.byref(ti), None))
        if not on.value:
            return None
        table = np.zeros((len(self._flat["materials"]), 3), f32)
        _lib.check(L.nt_scene_get_xray(self._handle, None, None, None, table.ctypes.data_as(_lib.f32p)))
        return dict(absorbance=float(ab.value), tint=float(ti.value), transmittance=table)

    def crossing_counts(self, width, height, device=None):
        """How many primitives the primary ray of every pixel of a width x height view of the scene's camera crosses
        (nt_crossing_counts; the rule: include/ntracer_hip.h), whether or not set_xray is on: int32 [height][width] -- a numpy
        array, or with `device` a torch device a torch tensor there, enqueued on torch's current stream."""
        return self._view_query("nt_crossing_counts", width, height, device, np.int32, None, None)

    def hit_layers(self, width, height, layers=4, device=None):
        """The `layers` (1..8) nearest surfaces under every pixel of a width x height view of the scene's camera, nearest first,
        with what each one is and the pixel's full crossing count (nt_hit_layers; the rule: include/ntracer_hip.h): a HitLayers
        of numpy arrays, or with `device` a torch device of torch tensors there, enqueued on torch's current stream.  One walk
        of the tree whatever `layers` is; opacity and every view setting but the camera play no part.  CompositeScene only."""
        if isinstance(layers, bool) or not isinstance(layers, (int, np.integer)) or not 1 <= layers <= 8:
            raise ValueError("layers must be an int in 1..8")
        layers = int(layers)
        width, height = int(width), int(height)
        if width < 1 or height < 1:
            raise ValueError("the size of a view must be positive")
        L = _lib.lib()
        opts = _lib.NtRenderOpts()
        if device is None:
            opts.device = -1
            out = np.zeros((layers, height, width, 4), np.int32)
            _lib.check(L.nt_hit_layers(self._handle, width, height, layers, out.ctypes.data, C.byref(opts)))
            return HitLayers(self, width, height, layers, out)
        import torch
        dev = torch.device(device)
        if dev.type != "cuda":
            raise ValueError("device must be a HIP device")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        opts.device = dev.index
        out = torch.empty((layers, height, width, 4), dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(L.nt_hit_layers_device(self._handle, width, height, layers, C.c_void_p(out.data_ptr()), C.byref(opts), C.c_void_p(stream)))
        return HitLayers(self, width, height, layers, out)

    def set_depth_cue(self, near=0.0, far=1.0, color=(0, 0, 0), strength=1.0, background=False, tint_axis=None, tint_range=None,
                      tint_colors=None):
        """Depth cues on the renders (include/ntracer_hip.h), from the primary hits of the render itself.  Fog: a
        pixel with an opaque hit at distance t fades towards `color` by strength * clamp01((t - near) / (far - near)), and with
        `background` so do the pixels that hit nothing at all, in full.  Tint ("colour by w"): with `tint_axis`, a Vector or n
        numbers, the pixel's plain colour is first multiplied by the colour between tint_colors = (colour_lo, colour_hi) at
        g = clamp01((axis . x - lo) / (hi - lo)), x the visible point and tint_range = (lo, hi); both are required exactly when
        tint_axis is given.  set_depth_cue(None) takes the setting off.  CompositeScene only.  Supersampling, row bands,
        statistics, a lens, the parallel projection, ambient occlusion and outlines are refused with it; calculate_color /
        colors_at, primary_hits, ray_colors, render_rays, the ray queries, refinement_mask, occlusion_counts and outline_mask
        ignore it.  A view setting like fov: not pickled."""
        L = _lib.lib()
        if near is None:
            _lib.check(L.nt_scene_set_depth_cue(self._handle, None, None))
            return
        cue, axis = _fog_and_tint(self.dimension, near, far, color, strength, background, tint_axis, tint_range, tint_colors)
        _lib.check(L.nt_scene_set_depth_cue(self._handle, C.byref(cue), None if axis is None else axis.ctypes.data_as(_lib.f32p)))

    @property
    def depth_cue(self):
        """None, or a dict of the setting: near, far, color, strength, background, and tint_axis, tint_range, tint_colors (None
        without a tint)"""
        on, tint, cue = C.c_int(0), C.c_int(0), _lib.NtDepthCue()
        axis = np.zeros(self.dimension, f32)
        _lib.check(_lib.lib().nt_scene_get_depth_cue(self._handle, C.byref(on), C.byref(cue), C.byref(tint), axis.ctypes.data_as(_lib.f32p)))
        if not on.value:
            return None
        return _fog_and_tint_dict(cue, tint.value, axis)

    def depth_cue_factors(self, width, height, device=None, strict_reference=None):
        """The two factors (f, g) of every pixel of a width x height view of the scene's camera under the setting that is on
        (nt_depth_cue_factors): float32 [height][width][2], f the fog factor and g the tint factor, -1 where the pixel carries
        none -- a numpy array, or with `device` a torch device a torch tensor there, enqueued on torch's current stream."""
        return self._view_query("nt_depth_cue_factors", width, height, device, f32, "depth_cue", "the depth cue is off (set_depth_cue)",
                                strict_reference, tail=(2,))

    def set_clip_planes(self, planes):
        """Cutaway views (include/ntracer_hip.h): `planes` is a sequence of up to 8 (normal, offset) pairs, a
        normal being a Vector or n numbers, finite and not all zero, and the keep-region the points x with normal . x <= offset
        for every pair (clip_plane_through makes a pair from a point and a normal).  Every ray of a render honours it -- primary,
        shadow and reflection rays, and the continuation through transparent hits -- so the geometry cut away casts no shadow and
        shows in no mirror; there are no caps.  render and primary_hits honour the setting.  set_clip_planes(None) or an empty
        sequence takes it off.  CompositeScene only.  Supersampling, row bands, statistics, a lens, the parallel projection,
        ambient occlusion, outlines, depth cues and scenes with Solids are refused with it, and so are calculate_color /
        colors_at, ray_colors, render_rays, refinement_mask, occlusion_counts, outline_mask and depth_cue_factors while it is on;
        the ray queries ignore it.  A view setting like fov: not pickled."""
        L = _lib.lib()
        if planes is None:
            _lib.check(L.nt_scene_set_clip_planes(self._handle, 0, None, None))
            return
        pairs = list(planes)
        n = self.dimension
        normals = np.zeros((max(len(pairs), 1), n), f32)
        offsets = np.zeros(max(len(pairs), 1), f32)
        for k, pair in enumerate(pairs):
            try:
                normal, offset = pair
            except (TypeError, ValueError):
                raise ValueError("a clip plane is a (normal, offset) pair")
            row = [float(v) for v in normal]
            if len(row) != n:
                raise ValueError("the normal of a clip plane must have %d components" % n)
            if isinstance(offset, bool) or not isinstance(offset, (int, float, np.integer, np.floating)):
                raise ValueError("the offset of a clip plane must be a number")
            normals[k] = row
            offsets[k] = offset
        _lib.check(L.nt_scene_set_clip_planes(self._handle, len(pairs), normals.ctypes.data_as(_lib.f32p), offsets.ctypes.data_as(_lib.f32p)))

    @property
    def clip_planes(self):
        """the setting of set_clip_planes: a tuple of (normal, offset) pairs, normal a tuple of n floats; empty while off"""
        count = C.c_int(0)
        normals = np.zeros((_lib.NT_CLIP_MAX, self.dimension), f32)
        offsets = np.zeros(_lib.NT_CLIP_MAX, f32)
        _lib.check(_lib.lib().nt_scene_get_clip_planes(self._handle, C.byref(count), normals.ctypes.data_as(_lib.f32p),
                                                       offsets.ctypes.data_as(_lib.f32p)))
        return tuple((tuple(float(v) for v in normals[k]), float(offsets[k])) for k in range(count.value))

    def set_lens(self, lens):
        """Render through `lens` (a Lens of the image's size) instead of the pinhole; None takes it off.  fov is ignored
        while a lens is set.  Supersampling, row bands, statistics, calculate_color / colors_at and primary_hits are refused
        under a lens; ray_colors, render_rays and the ray queries ignore it.  A view setting like fov: not pickled."""
        if lens is not None and not isinstance(lens, Lens):
            raise TypeError("lens must be a Lens or None")
        _lib.check(_lib.lib().nt_scene_set_lens(self._handle, lens._handle if lens is not None else None))
        self._lens = lens

    lens = property(lambda s: getattr(s, "_lens", None))

    def set_parallel_projection(self, half_width):
        """Render under the parallel (orthographic) projection: every pixel's ray runs along the camera's forward row and
        starts in the camera's image plane, which spans 2 * half_width scene units across with square pixels
        (include/ntracer_hip.h); None or 0 takes it off.  fov is ignored while it is set; a lens and the projection exclude
        each other (ValueError).  Supersampling, row bands, statistics, calculate_color / colors_at and primary_hits are
        refused under it; ray_colors, render_rays and the ray queries ignore it.  A view setting like fov: not pickled."""
        if half_width is None:
            half_width = 0.0
        if isinstance(half_width, bool) or not isinstance(half_width, (int, float, np.integer, np.floating)):
            raise ValueError("half_width must be a number or None")
        _lib.check(_lib.lib().nt_scene_set_parallel(self._handle, float(half_width)))

    @property
    def parallel_projection(self):
        """None, or the half_width of the parallel projection"""
        v = float(_lib.lib().nt_scene_get_parallel(self._handle))
        return v if v > 0.0 else None

    def parallel_rays(self, width, height, camera=None):
        """(origins float32 [height * width][n], direction float32 [n]): the rays a width x height render casts under the
        parallel projection that is set, for `camera` or the scene's own -- the origins computed in float32 in the device's
        operation order, the direction the unnormalised forward row.  With the direction repeated for every origin
        (np.broadcast_to(direction, origins.shape)) Scene.render_rays / ray_colors reproduce what the render casts."""
        hw = self.parallel_projection
        if hw is None:
            raise ValueError("no parallel projection is set")
        width, height = int(width), int(height)
        if width < 1 or height < 1:
            raise ValueError("the size of a view must be positive")
        if camera is None:
            camera = self.get_camera()
        elif not isinstance(camera, Camera) or camera.dimension != self._n:
            raise TypeError("the scene and camera must have the same dimension")
        org = np.ascontiguousarray(camera._origin, f32)
        ax = np.ascontiguousarray(camera._axes, f32)
        half_w, half_h = f32(width) / f32(2), f32(height) / f32(2)
        k = f32(hw) / half_w
        sx = (k * (np.arange(width, dtype=f32) - half_w)).astype(f32)
        sy = (k * (np.arange(height, dtype=f32) - half_h)).astype(f32)
        o = (org[None, None, :] + ax[0][None, None, :] * sx[None, :, None]) - ax[1][None, None, :] * sy[:, None, None]
        return np.ascontiguousarray(o.reshape(height * width, self._n), f32), ax[2].copy()

    def set_view_stack(self, offsets, focus=None, weights=None):
        """One picture from K cameras that differ from the scene's by a small offset, their plain pictures clamped, weighted and
        summed in fp32 on the device (include/ntracer_hip.h has the rule).  offsets: K rows of n floats in the
        camera's own frame (right, up, forward, the hidden axes); focus: None, or the distance of the plane on which all K rays of
        a pixel meet; weights: None for 1 / K each, or K rows of (r, g, b).  aperture_disc, slab and stereo_pair make the usual
        tables.  set_view_stack(None) takes the setting off.  A view setting like fov: not pickled."""
        L = _lib.lib()
        if offsets is None:
            _lib.check(L.nt_scene_set_view_stack(self._handle, 0, None, 0.0, None))
            return
        off = np.ascontiguousarray(offsets, f32)
        if off.ndim != 2 or off.shape[1] != self._n:
            raise ValueError("the offsets of a view stack are rows of %d floats" % self._n)
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, f32)
            if w.shape != (off.shape[0], 3):
                raise ValueError("the weights of a view stack are one (r, g, b) row a sample")
        if focus is not None and (isinstance(focus, bool) or not isinstance(focus, (int, float, np.integer, np.floating))):
            raise ValueError("focus must be a number or None")
        if focus is not None and not float(focus) > 0.0:
            raise ValueError("focus must be positive (None: no focus)")
        _lib.check(L.nt_scene_set_view_stack(self._handle, off.shape[0], off.ctypes.data_as(_lib.f32p), 0.0 if focus is None else float(focus),
                                             None if w is None else w.ctypes.data_as(_lib.f32p)))

    @property
    def view_stack(self):
        """None, or the setting of set_view_stack: a dict of offsets float32 [K][n], focus (None without one), weights [K][3]"""
        count, focus = C.c_int(0), C.c_float(0.0)
        off = np.zeros((_lib.NT_STACK_MAX, self._n), f32)
        w = np.zeros((_lib.NT_STACK_MAX, 3), f32)
        _lib.check(_lib.lib().nt_scene_get_view_stack(self._handle, C.byref(count), off.ctypes.data_as(_lib.f32p), C.byref(focus),
                                                      w.ctypes.data_as(_lib.f32p)))
        if count.value == 0:
            return None
        return {"offsets": off[:count.value].copy(), "focus": float(focus.value) if focus.value > 0.0 else None,
                "weights": w[:count.value].copy()}

    def set_view_stack_route(self, route):
        """A testing and measuring hook, not a feature.  None: a BoxScene of up to 24 dimensions draws its view stacks with the
        fused kernel (the default); "frames": through the fp32 scratch and the resolve pass, the route of every other scene.
        Same bytes either way: the suite and tools/view_stack_time.py hold the two routes against each other with it."""
        if route not in (None, "frames"):
            raise ValueError('the route of a view stack is None or "frames"')
        _lib.check(_lib.lib().nt_scene_set_view_stack_route(self._handle, _lib.NT_STACK_ROUTE_FRAMES if route else _lib.NT_STACK_ROUTE_AUTO))

    @property
    def view_stack_route(self):
        """None, or "frames" (set_view_stack_route)"""
        return "frames" if _lib.lib().nt_scene_get_view_stack_route(self._handle) == _lib.NT_STACK_ROUTE_FRAMES else None

    def view_stack_cameras(self, camera=None):
        """(origins float32 [K][n], axes float32 [K][n][n]): the K cameras the view stack that is set gives for `camera`, or for
        the scene's own -- computed on the host, bit for bit what the renders use"""
        vs = self.view_stack
        if vs is None:
            raise ValueError("no view stack is set")
        if camera is not None and (not isinstance(camera, Camera) or camera.dimension != self._n):
            raise TypeError("the scene and camera must have the same dimension")
        K = len(vs["offsets"])
        origins = np.zeros((K, self._n), f32)
        axes = np.zeros((K, self._n, self._n), f32)
        o = None if camera is None else np.ascontiguousarray(camera._origin, f32)
        a = None if camera is None else np.ascontiguousarray(camera._axes, f32)
        _lib.check(_lib.lib().nt_view_stack_cameras(self._handle, None if o is None else o.ctypes.data_as(_lib.f32p),
                                                    None if a is None else a.ctypes.data_as(_lib.f32p), origins.ctypes.data_as(_lib.f32p),
                                                    axes.ctypes.data_as(_lib.f32p)))
        return origins, axes

    def set_camera(self, camera):
        if not isinstance(camera, Camera) or camera.dimension != self._n:
            raise TypeError("the scene and camera must have the same dimension")
        o = np.ascontiguousarray(camera._origin, f32)
        a = np.ascontiguousarray(camera._axes, f32)
        _lib.check(_lib.lib().nt_scene_set_camera(self._handle, o.ctypes.data_as(_lib.f32p), a.ctypes.data_as(_lib.f32p)))

    def get_camera(self):
        c = Camera(self._n)
        o = np.zeros(self._n, f32)
        a = np.zeros((self._n, self._n), f32)
        _lib.check(_lib.lib().nt_scene_get_camera(self._handle, o.ctypes.data_as(_lib.f32p), a.ctypes.data_as(_lib.f32p)))
        c._origin, c._axes = o, a
        return c

    def _set_camera_arrays(self, origin, axes):
        o = np.ascontiguousarray(origin, f32)
        a = np.ascontiguousarray(axes, f32).reshape(self._n, self._n)
        _lib.check(_lib.lib().nt_scene_set_camera(self._handle, o.ctypes.data_as(_lib.f32p), a.ctypes.data_as(_lib.f32p)))

    def colors_at(self, xs, ys, width, height, device=-1):
        """fp32 colours of many pixels in one launch (batched Scene.calculate_color)."""
        xs = np.ascontiguousarray(xs, np.int32)
        ys = np.ascontiguousarray(ys, np.int32)
        out = np.zeros((len(xs), 3), f32)
        _lib.check(_lib.lib().nt_colors_at(self._handle, int(width), int(height), len(xs), xs.ctypes.data_as(_lib.i32p),
                                           ys.ctypes.data_as(_lib.i32p), out.ctypes.data_as(_lib.f32p), int(device)))
        return out

    def _rays_arg(self, origins, directions):
        """(nt_rays, count, torch device or None, arrays to keep alive) for ray_colors / render_rays"""
        n = self._n
        on_device = type(directions).__module__.split(".")[0] == "torch" and getattr(directions, "is_cuda", False)
        if on_device:
            import torch
            dev = directions.device
            for a in (origins, directions):
                if (type(a).__module__.split(".")[0] != "torch" or a.device != dev or a.dtype != torch.float32 or not a.is_contiguous()):
                    raise ValueError("device arrays of a ray batch must be contiguous %s tensors on %s" % (torch.float32, dev))
            ptr = lambda a: a.data_ptr()
        else:
            dev = None
            origins = np.ascontiguousarray(origins, f32)
            directions = np.ascontiguousarray(directions, f32)
            ptr = lambda a: a.ctypes.data
        if len(directions.shape) != 2 or int(directions.shape[1]) != n:
            raise ValueError("directions must have shape (count, %d)" % n)
        count = int(directions.shape[0])
        shared = tuple(origins.shape) == (n,)
        if not shared and tuple(origins.shape) != (count, n):
            raise ValueError("origins must have shape (count, %d) or (%d,)" % (n, n))
        rays = _lib.NtRays()
        rays.count, rays.origins, rays.directions, rays.shared_origin = count, ptr(origins), ptr(directions), 1 if shared else 0
        return rays, count, dev, (origins, directions)

    @staticmethod
    def _rays_opts(dev, strict_reference):
        opts = _lib.NtRenderOpts()
        opts.device = dev.index if dev.index is not None else -1
        if strict_reference is None:
            strict_reference = os.environ.get("NTRACER_STRICT_REFERENCE", "0") not in ("", "0")
        opts.strict_reference = 1 if strict_reference else 0
        return opts

    def ray_colors(self, origins, directions, device=-1, out=None, strict_reference=None):
        """fp32 colours of the caller's own rays (nt_ray_colors): ray_color at depth 0 -- BoxScene: calculate_color -- for each
        (origin, direction), the direction normalised as the camera's ray source normalises its own; the scene's camera, fov
        and supersampling factor play no part.  origins [count][n], or [n] for one origin shared by every ray; directions
        [count][n], any non-zero finite length.  numpy arrays in: a numpy [count][3] float32 array out, through host memory.
        Contiguous float32 torch tensors on a HIP device in: a torch tensor on that device (or `out`, the caller's own
        [count][3]), enqueued on torch's current stream without a copy or a synchronisation."""
        rays, count, dev, keep = self._rays_arg(origins, directions)
        L = _lib.lib()
        if dev is None:
            if out is None:
                out = np.zeros((count, 3), f32)
            elif not (isinstance(out, np.ndarray) and out.dtype == f32 and out.shape == (count, 3) and out.flags.c_contiguous and out.flags.writeable):
                raise ValueError("out must be a writable contiguous float32 array of shape (%d, 3)" % count)
            _lib.check(L.nt_ray_colors(self._handle, C.byref(rays), out.ctypes.data, int(device)))
            return out
        import torch
        if out is None:
            out = torch.zeros((count, 3), dtype=torch.float32, device=dev)
        elif (type(out).__module__.split(".")[0] != "torch" or out.device != dev or out.dtype != torch.float32 or not out.is_contiguous()
              or tuple(out.shape) != (count, 3)):
            raise ValueError("out must be a contiguous %s tensor of shape %r on %s" % (torch.float32, (count, 3), dev))
        if count == 0:
            return out                          # (an empty tensor has no address to hand over)
        opts = self._rays_opts(dev, strict_reference)
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(L.nt_ray_colors_device(self._handle, C.byref(rays), out.data_ptr(), C.byref(opts), stream))
        return out

    def render_rays(self, dest, format, origins, directions, device=-1, strict_reference=None):
        """The image whose pixel (x, y) is the colour of ray y * width + x (nt_render_rays), packed in `format` as
        BlockingRenderer.render packs a frame.  `dest`: a writable buffer, with numpy rays -- or a torch uint8 tensor on the
        device, with device rays, enqueued on torch's current stream."""
        if not isinstance(format, _render.ImageFormat):
            raise TypeError("format must be an ImageFormat")
        rays, count, dev, keep = self._rays_arg(origins, directions)
        fmt = format._as_struct()
        L = _lib.lib()
        target = _render._device_pointer(dest)
        if (target is None) != (dev is None):
            raise ValueError("the destination and the rays must both be in host memory or both on the device")
        if dev is None:
            arr, nbytes = _render._host_buffer(dest)
            _lib.check(L.nt_render_rays(self._handle, arr, nbytes, C.byref(fmt), C.byref(rays), int(device)))
            return True
        ptr, nbytes, index, stream = target
        if index != dev.index:
            raise ValueError("the destination and the rays must be on the same device")
        opts = self._rays_opts(dev, strict_reference)
        _lib.check(L.nt_render_rays_device(self._handle, C.c_void_p(ptr), nbytes, C.byref(fmt), C.byref(rays), C.byref(opts), C.c_void_p(stream)))
        return True

    def last_stats(self):
        st = _lib.NtStats()
        _lib.check(_lib.lib().nt_scene_last_stats(self._handle, C.byref(st)))
        return st.as_dict()


class BoxScene(_SceneBase):
    """tracern.BoxScene(dimension) -- one hypercube [-1,1]^n (tracer.hpp:83-123)."""

    def __init__(self, dimension):
        n = int(dimension)
        h = _lib.lib().nt_box_scene_create(n)
        if not h:
            raise ValueError(_lib.last_error())
        self._handle = h
        self._init_common(n)

    def face_hits(self, width, height, device=-1, out=None, table=None, first=0, count=None, frame_stride=None):
        """Which face of the cube is under each pixel of a width x height view, and how far away (nt_box_hits; the rule in full:
        include/ntracer_hip.h).  Returns a FaceHits: dist, axis, side, hit, each [height][width], and records.

        `device` an int: numpy arrays through host memory, the scene's current camera.  `device` a torch device (or `out`
        given): torch tensors that stay on the device, enqueued on torch's current stream without a synchronisation.  `out`:
        the caller's own contiguous int32 tensor [frames * frame_stride][4].  `table` (a render.CameraTable): frames
        [first, first + count) of it in one launch, every array [count][height][width], `frame_stride` >= width * height
        records between the frames, whose records in between are not touched (torch only: the table lives on a device)."""
        width, height = int(width), int(height)
        if width < 1 or height < 1:
            raise ValueError("the view must be at least 1 x 1")
        per_frame = width * height
        torch_device = device if type(device).__module__.split(".")[0] == "torch" or isinstance(device, str) else None
        on_device = torch_device is not None or out is not None or table is not None
        L = _lib.lib()
        if not on_device:
            recs = np.zeros((per_frame, 4), np.int32)
            _lib.check(L.nt_box_hits(self._handle, width, height, recs.ctypes.data, int(device)))
            return FaceHits(self._n, width, height, None, per_frame, recs)
        import torch
        frames = 1
        if table is not None:
            first = int(first)
            frames = table.frames - first if count is None else int(count)
        stride = per_frame if frame_stride is None else int(frame_stride)
        if stride < per_frame or (table is None and stride != per_frame):
            raise ValueError("frame_stride must be at least width * height (and is only taken with a camera table)")
        if out is not None:
            dev = out.device
        elif torch_device is not None:
            dev = torch.device(torch_device)
        else:
            dev = torch.device("cuda", torch.cuda.current_device() if int(device) < 0 else int(device))
        if dev.type != "cuda":
            raise ValueError("device must be a HIP device")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        shape = (frames * stride, 4)
        if out is None:
            recs = torch.zeros(shape, dtype=torch.int32, device=dev)          # (zeroed on the stream)
        else:
            recs = out
            if recs.dtype != torch.int32 or not recs.is_contiguous() or tuple(recs.shape) != shape:
                raise ValueError("out must be a contiguous int32 tensor of shape %r on %s" % (shape, dev))
        opts = _lib.NtRenderOpts()
        opts.device = dev.index
        stream = torch.cuda.current_stream(dev).cuda_stream
        if table is None:
            _lib.check(L.nt_box_hits_device(self._handle, width, height, C.c_void_p(recs.data_ptr()), C.byref(opts), C.c_void_p(stream)))
        else:
            _lib.check(L.nt_box_hits_table_device(self._handle, width, height, C.c_void_p(recs.data_ptr()), stride, table._h, first, frames,
                                                  C.byref(opts), C.c_void_p(stream)))
        return FaceHits(self._n, width, height, None if table is None else frames, stride, recs)

    def set_face_lines(self, color=(0, 0, 0), strength=1.0, silhouette=True, edges=True):
        """Draw a line along the cube's silhouette and along every edge where two of its faces meet, inside the render
        (include/ntracer_hip.h).  A pixel that sees a face is marked when one of its four neighbours sees nothing
        (`silhouette`) or sees another face that is not nearer (`edges`); a marked pixel's plain colour P becomes
        P * (1 - strength) + color * strength.  set_face_lines(None) takes the setting off.  Supersampling, row bands,
        statistics, a lens and the parallel projection are refused with it; calculate_color / colors_at, face_hits, ray_colors,
        render_rays and refinement_mask ignore it.  A view setting like fov: not pickled."""
        L = _lib.lib()
        if color is None:
            _lib.check(L.nt_scene_set_box_lines(self._handle, 0, None, 0.0))
            return
        if isinstance(strength, bool) or not isinstance(strength, (int, float, np.integer, np.floating)):
            raise ValueError("strength must be a number")
        col = np.ascontiguousarray([float(c) for c in color], f32)
        if col.shape != (3,):
            raise ValueError("color must have three components")
        kinds = (_lib.NT_OUTLINE_SILHOUETTE if silhouette else 0) | (_lib.NT_OUTLINE_CREASE if edges else 0)
        if not kinds:
            raise ValueError("face lines without silhouette and edges: set_face_lines(None) takes the setting off")
        _lib.check(L.nt_scene_set_box_lines(self._handle, kinds, col.ctypes.data_as(_lib.f32p), float(strength)))

    @property
    def face_lines(self):
        """None, or a dict of the setting: silhouette, edges, color (three floats), strength"""
        kinds, st = C.c_int(0), C.c_float(0.0)
        col = np.zeros(3, f32)
        _lib.check(_lib.lib().nt_scene_get_box_lines(self._handle, C.byref(kinds), col.ctypes.data_as(_lib.f32p), C.byref(st)))
        if not kinds.value:
            return None
        return dict(silhouette=bool(kinds.value & _lib.NT_OUTLINE_SILHOUETTE), edges=bool(kinds.value & _lib.NT_OUTLINE_CREASE),
                    color=tuple(float(c) for c in col), strength=float(st.value))

    def set_face_shading(self, colors=None, *, near=None, far=None, color=(0, 0, 0), strength=1.0, background=False, tint_axis=None,
                         tint_range=None, tint_colors=None):
        """Shade the cube's faces from the face records of the render itself (include/ntracer_hip.h): `colors`, an
        [n][2][3] array-like with components in [0, 1], gives each of the 2n faces a colour of its own -- colors[i][1] the face
        at +1 of axis i, colors[i][0] the face at -1; face_palette(n) makes one -- in place of the one (1, 0.5, 0.5).  The other
        arguments are CompositeScene.set_depth_cue's: fog from `near` to `far` towards `color` by `strength`, on the background
        too with `background`, and a tint along `tint_axis` with tint_range = (lo, hi) and tint_colors = (colour_lo, colour_hi).
        Without fog arguments the fog has strength 0 (near, far = 0, 1).  `near` without `far`, and `color`, `strength` or
        `background` other than their defaults without `far`, are a ValueError: nothing is dropped silently.  With
        set_face_lines on as well the lines are drawn on top. set_face_shading(None) with nothing else takes the setting off.  Supersampling, row bands, statistics, a lens and
        the parallel projection are refused with it; calculate_color / colors_at, face_hits, face_line_mask, ray_colors,
        render_rays and refinement_mask ignore it.  A view setting like fov: not pickled."""
        L = _lib.lib()
        table = None
        if colors is not None:
            table = np.ascontiguousarray(colors, f32)
            if table.shape != (self.dimension, 2, 3):
                raise ValueError("colors must have the shape (%d, 2, 3)" % self.dimension)
        fog = near is not None or far is not None
        if not fog and (tuple(color) != (0, 0, 0) or isinstance(strength, bool) or strength != 1.0 or background):
            raise ValueError("color, strength and background are the fog's: they need far")
        if not fog and tint_axis is None:
            if tint_range is not None or tint_colors is not None:
                raise ValueError("tint_range and tint_colors need a tint_axis")
            _lib.check(L.nt_scene_set_box_shading(self._handle, None if table is None else table.ctypes.data_as(_lib.f32p), None, None))
            return
        if fog and far is None:
            raise ValueError("a fog needs far (near is 0 without one)")
        cue, axis = _fog_and_tint(self.dimension, (0.0 if near is None else near) if fog else 0.0, far if fog else 1.0, color,
                                  strength if fog else 0.0, background if fog else False, tint_axis, tint_range, tint_colors)
        _lib.check(L.nt_scene_set_box_shading(self._handle, None if table is None else table.ctypes.data_as(_lib.f32p), C.byref(cue),
                                              None if axis is None else axis.ctypes.data_as(_lib.f32p)))

    @property
    def face_shading(self):
        """None, or a dict of the setting: colors (an [n][2][3] float32 array, None without a table of the caller's own), and near,
        far, color, strength, background, tint_axis, tint_range, tint_colors as CompositeScene.depth_cue has them (all None
        without fog and tint; the tint's three None without a tint)"""
        on, has_colors, has_fog, tint, cue = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), _lib.NtDepthCue()
        table = np.zeros((self.dimension, 2, 3), f32)
        axis = np.zeros(self.dimension, f32)
        _lib.check(_lib.lib().nt_scene_get_box_shading(self._handle, C.byref(on), C.byref(has_colors), table.ctypes.data_as(_lib.f32p),
                                                       C.byref(has_fog), C.byref(cue), C.byref(tint), axis.ctypes.data_as(_lib.f32p)))
        if not on.value:
            return None
        d = dict(colors=table if has_colors.value else None)
        if has_fog.value:
            d.update(_fog_and_tint_dict(cue, tint.value, axis))
        else:
            d.update(near=None, far=None, color=None, strength=None, background=None, tint_axis=None, tint_range=None, tint_colors=None)
        return d

    def face_line_mask(self, width, height, device=None):
        """The face-line mask of a width x height view of the scene's camera under the setting that is on (nt_box_line_mask):
        uint8 [height][width], 0 or an OR of NT_OUTLINE_SILHOUETTE and NT_OUTLINE_CREASE -- a numpy array, or with `device` a
        torch device a torch tensor there, enqueued on torch's current stream."""
        return self._view_query("nt_box_line_mask", width, height, device, np.uint8, "face_lines", "face lines are off (set_face_lines)",
                                counted=True, plain=True)


def face_palette(n):
    """A face-colour table for BoxScene.set_face_shading: float32 [n][2][3], one hue per axis, spread evenly round the colour
    circle from red; the face at +1 ([i][1]) at full value, the face at -1 ([i][0]) at half of it."""
    import colorsys
    n = int(n)
    if n < 1:
        raise ValueError("n must be at least 1")
    table = np.zeros((n, 2, 3), f32)
    for i in range(n):
        table[i, 1] = colorsys.hsv_to_rgb(i / n, 1.0, 1.0)
        table[i, 0] = colorsys.hsv_to_rgb(i / n, 1.0, 0.5)
    return table


def _fog_and_tint(dimension, near, far, color, strength, background, tint_axis, tint_range, tint_colors):
    """(nt_depth_cue, the tint axis as a float32 array or None) of the fog and tint arguments that CompositeScene.set_depth_cue
    and BoxScene.set_face_shading share"""
    for v in (near, far, strength):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError("near, far and strength must be numbers")

    def colour(c, what):
        col = [float(v) for v in c]
        if len(col) != 3:
            raise ValueError("%s must have three components" % what)
        return col

    cue = _lib.NtDepthCue()
    cue.fog_near, cue.fog_far, cue.fog_strength = float(near), float(far), float(strength)
    cue.fog_color[:] = colour(color, "color")
    cue.fog_background = 1 if background else 0
    axis = None
    if tint_axis is None:
        if tint_range is not None or tint_colors is not None:
            raise ValueError("tint_range and tint_colors need a tint_axis")
    else:
        if tint_range is None or tint_colors is None:
            raise ValueError("a tint_axis needs tint_range and tint_colors")
        axis = np.ascontiguousarray([float(v) for v in tint_axis], f32)
        if axis.shape != (dimension,):
            raise ValueError("tint_axis must have %d components" % dimension)
        lo, hi = tint_range
        cue.tint_lo, cue.tint_hi = float(lo), float(hi)
        c_lo, c_hi = tint_colors
        cue.tint_color_lo[:] = colour(c_lo, "tint_colors[0]")
        cue.tint_color_hi[:] = colour(c_hi, "tint_colors[1]")
    return cue, axis


def _fog_and_tint_dict(cue, tint, axis):
    d = dict(near=float(cue.fog_near), far=float(cue.fog_far), color=tuple(float(c) for c in cue.fog_color),
             strength=float(cue.fog_strength), background=bool(cue.fog_background), tint_axis=None, tint_range=None, tint_colors=None)
    if tint:
        d.update(tint_axis=tuple(float(v) for v in axis), tint_range=(float(cue.tint_lo), float(cue.tint_hi)),
                 tint_colors=(tuple(float(c) for c in cue.tint_color_lo), tuple(float(c) for c in cue.tint_color_hi)))
    return d


_FLAT_KEYS = ("root", "node_axis", "node_split", "node_left", "node_right", "items", "batch_recs", "batch_mats",
              "tri_recs", "tri_mats", "solid_recs", "solid_types", "solid_mats", "materials", "aabb_start", "aabb_end")


class CompositeScene(_SceneBase):
    """tracern.CompositeScene(boundary,data) -- the contents of a k-d tree (tracer.hpp:1710-1927)."""

    def __init__(self, boundary, data):
        if not isinstance(boundary, AABB):
            raise TypeError("boundary must be an AABB")
        if not isinstance(data, KDNode):
            raise TypeError("data must be a KDNode")
        if boundary.dimension != data.dimension:
            raise TypeError("boundary and data must have the same dimension")
        self._create(self._flatten(boundary, data))
        self._root_obj = data
        data._owner = weakref.ref(self)

    @classmethod
    def _for_node(cls, boundary, node):
        """the private scene of a node that is no scene's root (KDNode._query_scene)"""
        self = object.__new__(cls)
        self._create(cls._flatten(boundary, node))
        self._root_obj = node
        return self

    @classmethod
    def from_flat(cls, dimension, flat):
        """Build directly from flat arrays (the layout of nt_scene_desc / tests/golden/*.npz)."""
        self = object.__new__(cls)
        d = {k: flat[k] for k in _FLAT_KEYS}
        d["dimension"] = int(dimension)
        self._create(d)
        return self

    @staticmethod
    def _flatten(boundary, root):
        n = boundary.dimension
        nodes, items = [], []
        batch_ids, tri_ids, solid_ids, mat_ids = {}, {}, {}, {}
        batch_recs, batch_mats, tri_recs, tri_mats, solid_recs, solid_types, solid_mats, mats = [], [], [], [], [], [], [], []
        objects = ([], [], [])            # item -> the caller's object, per kind (RayIntersection.primitive)

        def mat(m):
            k = m._key()
            if k not in mat_ids:
                mat_ids[k] = len(mats)
                mats.append(list(m.color) + list(m.specular) + [m.opacity, m.reflectivity, m.specular_intensity, m.specular_exp])
            return mat_ids[k]

        def item(p):
            if isinstance(p, TriangleBatch):
                if id(p) not in batch_ids:
                    batch_ids[id(p)] = len(batch_recs)
                    objects[_lib.KIND_BATCH].append(p)
                    batch_recs.append([t._record() for t in p._tris])
                    batch_mats.append([mat(t.material) for t in p._tris])
                return (batch_ids[id(p)] << 2) | _lib.KIND_BATCH
            if isinstance(p, Triangle):
                if id(p) not in tri_ids:
                    tri_ids[id(p)] = len(tri_recs)
                    objects[_lib.KIND_TRIANGLE].append(p)
                    tri_recs.append(p._record())
                    tri_mats.append(mat(p.material))
                return (tri_ids[id(p)] << 2) | _lib.KIND_TRIANGLE
            if id(p) not in solid_ids:
                solid_ids[id(p)] = len(solid_recs)
                objects[_lib.KIND_SOLID].append(p)
                solid_recs.append(np.concatenate([p.orientation._m.ravel(), p.inv_orientation._m.ravel(), p.position._v]))
                solid_types.append(p.type)
                solid_mats.append(mat(p.material))
            return (solid_ids[id(p)] << 2) | _lib.KIND_SOLID

        def add(node):
            if node is None:
                return -1
            if node.dimension != n:
                raise TypeError("boundary and data must have the same dimension")
            idx = len(nodes)
            nodes.append(None)
            if isinstance(node, KDLeaf):
                start = len(items)
                for p in node._items:
                    items.append(item(p))
                nodes[idx] = (-1, 0.0, start, len(node._items))
            else:
                l = add(node.left)
                r = add(node.right)
                nodes[idx] = (node.axis, node.split, l, r)
            return idx

        root_idx = add(root)
        nd = np.asarray(nodes, np.float64).reshape(-1, 4)
        rl = n * n + n + 1
        return dict(dimension=n, root=root_idx, _objects=objects,
                    node_axis=nd[:, 0].astype(np.int32), node_split=nd[:, 1].astype(f32),
                    node_left=nd[:, 2].astype(np.int32), node_right=nd[:, 3].astype(np.int32),
                    items=np.asarray(items, np.int32),
                    batch_recs=np.asarray(batch_recs, f32).reshape(-1, BATCH_SIZE, rl),
                    batch_mats=np.asarray(batch_mats, np.int32).reshape(-1, BATCH_SIZE),
                    tri_recs=np.asarray(tri_recs, f32).reshape(-1, rl), tri_mats=np.asarray(tri_mats, np.int32),
                    solid_recs=np.asarray(solid_recs, f32).reshape(-1, 2 * n * n + n),
                    solid_types=np.asarray(solid_types, np.int32), solid_mats=np.asarray(solid_mats, np.int32),
                    materials=np.asarray(mats, f32).reshape(-1, 10),
                    aabb_start=boundary.start._v, aabb_end=boundary.end._v)

    def with_rebuilt_tree(self, **kwds):
        """A new CompositeScene over the SAME primitive tables (batches, triangles, solids, materials -- so the same
        pixels: nearest hits do not depend on the tree) with the k-d tree rebuilt by the native builder.  Keyword
        arguments as for build_kdtree (max_depth, split_threshold, traversal_cost, intersection_cost).  Scene
        parameters (lights, background, fov, camera) are copied.  With shadows on the pixels DO depend on the tree,
        here as in the reference: its occlusion walk skips the far child of a branch whenever the split lies nearer
        than the light (tracer.hpp:1298), so a different tree finds different blockers."""
        f = self._flat
        n = self.dimension
        items = []
        brec = np.asarray(f["batch_recs"], np.float64).reshape(-1, BATCH_SIZE, n * n + n + 1)
        if len(brec):
            bv = builder.vertices_of_many(brec.reshape(-1, brec.shape[2]), n).reshape(len(brec), BATCH_SIZE, n, n)
            for k in range(len(brec)):
                items.append(builder._Item((k << 2) | _lib.KIND_BATCH, bv[k].min(axis=(0, 1)), bv[k].max(axis=(0, 1)), bv[k]))
        trec = np.asarray(f["tri_recs"], np.float64).reshape(-1, n * n + n + 1)
        if len(trec):
            tv = builder.vertices_of_many(trec, n)
            for k in range(len(trec)):
                items.append(builder._Item((k << 2) | _lib.KIND_TRIANGLE, tv[k].min(axis=0), tv[k].max(axis=0), tv[k][None]))
        srec = np.asarray(f["solid_recs"], np.float64).reshape(-1, 2 * n * n + n)
        for k in range(len(srec)):
            lo, hi = builder.solid_bounds(int(f["solid_types"][k]) == CUBE, srec[k, 2 * n * n:], srec[k, :n * n].reshape(n, n))
            items.append(builder._Item((k << 2) | _lib.KIND_SOLID, lo, hi))
        nodes, leaf_items = [], []

        def leaf(prims):
            nodes.append([-1, 0.0, len(leaf_items), len(prims)])
            leaf_items.extend(prims)
            return len(nodes) - 1

        def branch(axis, split, left, right):
            nodes.append([axis, split, -1 if left is None else left, -1 if right is None else right])
            return len(nodes) - 1

        lo, hi, root = builder.build_tree(items, leaf, branch, int(kwds.pop("max_depth", builder.KD_DEFAULT_MAX_DEPTH)),
                                          int(kwds.pop("split_threshold", builder.KD_DEFAULT_SPLIT_THRESHOLD)),
                                          float(kwds.pop("traversal_cost", 0.0)), float(kwds.pop("intersection_cost", 0.0)))
        if kwds:
            raise TypeError("unexpected keyword argument %r" % next(iter(kwds)))
        nd = np.asarray(nodes, np.float64).reshape(-1, 4)
        d = {k: np.array(v) for k, v in f.items()}
        d.update(root=root, node_axis=nd[:, 0].astype(np.int32), node_split=nd[:, 1].astype(f32),
                 node_left=nd[:, 2].astype(np.int32), node_right=nd[:, 3].astype(np.int32),
                 items=np.asarray(leaf_items, np.int32), aabb_start=lo, aabb_end=hi)
        other = CompositeScene.from_flat(n, d)
        other.set_fov(self.fov)
        other.set_supersampling(self.supersampling)
        other.set_supersampling_scratch_mb(self.supersampling_scratch_mb)
        other.set_adaptive_supersampling(self.adaptive_supersampling)
        other._push(_pl=list(self._point_lights), _gl=list(self._global_lights), **dict(self._p))
        cam = self.get_camera()
        other._set_camera_arrays(cam._origin, cam._axes)
        return other

    @property
    def root(self):
        """CompositeScene.root (ntracer_body.hpp:922-924): the k-d tree as KDBranch / KDLeaf objects over Triangle,
        TriangleBatch and Solid objects.  Scenes made from flat arrays (build_composite_scene, from_flat) only
        materialise these when asked."""
        if getattr(self, "_root_obj", None) is not None:
            return self._root_obj
        f = self._flat
        n = self._n
        rl = n * n + n + 1
        mats = [Material.__new__(Material) for _ in range(len(f["materials"]))]
        for m, v in zip(mats, np.asarray(f["materials"], np.float64).reshape(-1, 10)):
            m.color = Color(*v[0:3])
            m.specular = Color(*v[3:6])
            m.opacity, m.reflectivity, m.specular_intensity, m.specular_exp = (float(x) for x in v[6:10])

        def tri(rec, mi):
            rec = np.asarray(rec, f32)
            return Triangle(rec[1 + n:1 + 2 * n], rec[1:1 + n], rec[1 + 2 * n:rl].reshape(n - 1, n), mats[int(mi)])

        brecs = np.asarray(f["batch_recs"], f32).reshape(-1, BATCH_SIZE, rl)
        bmats = np.asarray(f["batch_mats"], np.int64).reshape(-1, BATCH_SIZE)
        batches = [TriangleBatch([tri(brecs[k, l], bmats[k, l]) for l in range(BATCH_SIZE)]) for k in range(len(brecs))]
        trecs = np.asarray(f["tri_recs"], f32).reshape(-1, rl)
        tris = [tri(trecs[k], f["tri_mats"][k]) for k in range(len(trecs))]
        srecs = np.asarray(f["solid_recs"], f32).reshape(-1, 2 * n * n + n)
        solids = [Solid(int(f["solid_types"][k]), srecs[k, 2 * n * n:], Matrix._wrap(srecs[k, :n * n].reshape(n, n)), mats[int(f["solid_mats"][k])])
                  for k in range(len(srecs))]
        for k, sol in enumerate(solids):       # the inverse the scene was made with, not a recomputed one
            sol.inv_orientation = Matrix._wrap(srecs[k, n * n:2 * n * n].reshape(n, n))
        tables = (batches, tris, solids)
        self._objects = tables
        axis, split, left, right, items = f["node_axis"], f["node_split"], f["node_left"], f["node_right"], f["items"]
        made = {}
        order, stack = [], [int(f["root"])] if int(f["root"]) >= 0 else []
        while stack:
            k = stack.pop()
            order.append(k)
            if axis[k] >= 0:
                stack.extend(int(c) for c in (left[k], right[k]) if c >= 0)
        for k in reversed(order):
            if axis[k] < 0:
                made[k] = KDLeaf([tables[int(it) & 3][int(it) >> 2] for it in items[int(left[k]):int(left[k]) + int(right[k])]])
            else:
                made[k] = KDBranch(int(axis[k]), float(split[k]), made.get(int(left[k])), made.get(int(right[k])))
        self._root_obj = made.get(int(f["root"]))
        if self._root_obj is not None:
            self._root_obj._owner = weakref.ref(self)      # its queries run on this scene's handle
        return self._root_obj

    def _flat_description(self):
        """The flat arrays this scene was created from (layout of nt_scene_desc / tests/golden/*.npz)."""
        return {k: np.array(v) for k, v in self._flat.items()}

    def _create(self, d):
        self._flat = {k: np.array(d[k]) for k in _FLAT_KEYS}
        self._objects = d.get("_objects")          # item -> object tables; scenes from flat arrays make them with `root`
        self._item_ids = None
        n = int(d["dimension"])
        rl = n * n + n + 1
        keep = {}

        def fa(k, shape=None):
            a = np.ascontiguousarray(d[k], f32)
            if shape is not None:
                a = a.reshape(shape)
            keep[k] = a
            return a

        def ia(k):
            a = np.ascontiguousarray(d[k], np.int32)
            keep[k] = a
            return a

        desc = _lib.NtSceneDesc()
        desc.dimension = n
        desc.root = int(d["root"])
        na = ia("node_axis")
        desc.n_nodes = len(na)
        desc.node_axis = na.ctypes.data_as(_lib.i32p)
        desc.node_split = fa("node_split").ctypes.data_as(_lib.f32p)
        desc.node_left = ia("node_left").ctypes.data_as(_lib.i32p)
        desc.node_right = ia("node_right").ctypes.data_as(_lib.i32p)
        it = ia("items")
        desc.n_items = len(it)
        desc.items = it.ctypes.data_as(_lib.i32p)
        br = fa("batch_recs", (-1, BATCH_SIZE, rl))
        desc.n_batches = br.shape[0]
        desc.batch_recs = br.ctypes.data_as(_lib.f32p)
        bm = ia("batch_mats")
        if bm.size != br.shape[0] * BATCH_SIZE:
            raise ValueError("batch_mats does not match batch_recs")
        desc.batch_mats = bm.ctypes.data_as(_lib.i32p)
        tr = fa("tri_recs", (-1, rl))
        desc.n_triangles = tr.shape[0]
        desc.tri_recs = tr.ctypes.data_as(_lib.f32p)
        tm = ia("tri_mats")
        if tm.size != tr.shape[0]:
            raise ValueError("tri_mats does not match tri_recs")
        desc.tri_mats = tm.ctypes.data_as(_lib.i32p)
        sr = fa("solid_recs", (-1, 2 * n * n + n))
        desc.n_solids = sr.shape[0]
        desc.solid_recs = sr.ctypes.data_as(_lib.f32p)
        st = ia("solid_types")
        sm = ia("solid_mats")
        if st.size != sr.shape[0] or sm.size != sr.shape[0]:
            raise ValueError("solid arrays do not match")
        desc.solid_types = st.ctypes.data_as(_lib.i32p)
        desc.solid_mats = sm.ctypes.data_as(_lib.i32p)
        mt = fa("materials", (-1, 10))
        marr = (_lib.NtMaterial * max(len(mt), 1))()
        for i, r in enumerate(mt):
            marr[i].color[:] = [float(v) for v in r[0:3]]
            marr[i].specular[:] = [float(v) for v in r[3:6]]
            marr[i].opacity, marr[i].reflectivity, marr[i].specular_intensity, marr[i].specular_exp = [float(v) for v in r[6:10]]
        desc.n_materials = len(mt)
        desc.materials = marr
        a0 = fa("aabb_start", (n,))
        a1 = fa("aabb_end", (n,))
        desc.aabb_start = a0.ctypes.data_as(_lib.f32p)
        desc.aabb_end = a1.ctypes.data_as(_lib.f32p)
        h = _lib.lib().nt_composite_scene_create(C.byref(desc))
        if not h:
            raise ValueError(_lib.last_error())
        self._handle = h
        self._init_common(n)
        self.boundary = AABB(n, a0, a1)
        # composite_scene defaults (tracer.hpp:1727-1740)
        self._p = dict(shadows=False, camera_light=True, max_reflect_depth=4, bg_gradient_axis=1,
                       ambient=Color(0, 0, 0), bg1=Color(1, 1, 1), bg2=Color(0, 0, 0), bg3=Color(0, 1, 1))
        self._point_lights = []
        self._global_lights = []

    # ---- ray queries (nt_intersect_rays / nt_occludes_rays, include/ntracer_hip.h) ----
    def _object_of(self, kind, index):
        """the Triangle / TriangleBatch / Solid object behind a leaf item"""
        if self._objects is None:
            self.root                              # (materialises the tables of a scene made from flat arrays)
        return self._objects[kind][index]

    def _item_of(self, obj):
        """the leaf-item code of one of the scene's objects; -1 for anything else (it then matches nothing)"""
        if self._objects is None:
            self.root
        if self._item_ids is None:
            self._item_ids = {id(p): (i << 2) | kind for kind, tab in enumerate(self._objects) for i, p in enumerate(tab)}
        return self._item_ids.get(id(obj), -1)

    def _transparent_hits(self, o, d, recs, count):
        """RayIntersection objects for the first `count` records (dist, item, lane, -) of a ray's transparent list.  The
        kernels hand out what was hit and where along the ray; the normal ray a test would have written (triangle::intersects,
        tracer.hpp:431-437; solid::intersects, :251-276 with hypercube_intersects / hypersphere_intersects, :126-173) is
        worked out here, in fp32 with the reference's operations in the reference's order."""
        n = self._n
        o, d = np.asarray(o, f32), np.asarray(d, f32)

        def dot(a, b):                         # summed left to right, every step rounded to fp32
            acc = f32(a[0] * b[0])
            for k in range(1, len(a)):
                acc = f32(acc + f32(a[k] * b[k]))
            return acc

        out = []
        for rec in recs[:min(count, len(recs))]:
            dist = rec[0:1].view(f32)[0]
            item, lane = int(rec[1]), int(rec[2])
            kind, index = item & 3, item >> 2
            prim = self._object_of(kind, index)
            if kind == _lib.KIND_SOLID:
                orient, inv, pos = (np.asarray(a, f32) for a in (prim.orientation._m, prim.inv_orientation._m, prim.position._v))
                lo = np.asarray([f32(dot(inv[i], o) - pos[i]) for i in range(n)], f32)
                ld = np.asarray([dot(inv[i], d) for i in range(n)], f32)
                if prim.type == CUBE:
                    ln_o, ln_d = np.zeros(n, f32), np.zeros(n, f32)
                    for i in range(n):         # the first axis whose face the local ray passes through
                        if ld[i] == 0:
                            continue
                        s = f32(1.0 if ld[i] < 0 else -1.0)
                        t = f32(f32(s - lo[i]) / ld[i])
                        if not t > 0:
                            continue
                        p = (ld * t + lo).astype(f32)
                        if all(j == i or not abs(p[j]) > f32(1.0) + f32(_ROUNDING_FUZZ) for j in range(n)):
                            ln_o = p.copy()
                            ln_o[i] = s
                            ln_d[i] = s
                            break
                else:
                    ln_o = (lo + (ld * dist).astype(f32)).astype(f32)
                    ln_d = ln_o.copy()
                tmp = (ln_o + pos).astype(f32)
                origin = np.asarray([dot(orient[i], tmp) for i in range(n)], f32)
                normal = np.asarray([dot(orient[i], ln_d) for i in range(n)], f32)
            else:
                tri = prim[lane] if kind == _lib.KIND_BATCH else prim
                fn = np.asarray(tri.face_normal._v, f32)
                origin = (o + (d * dist).astype(f32)).astype(f32)
                normal = (fn / f32(np.sqrt(dot(fn, fn)))).astype(f32)
                if dot(fn, d) > 0:
                    normal = -normal
            out.append(RayIntersection(float(dist), Vector._wrap(origin), Vector._wrap(normal), prim, lane))
        return out

    def _ray_query(self, occlusion, origins, directions, t_near, t_far, distance, skip_item, skip_lane, normals, max_transparent, device):
        n = self._n
        max_transparent = int(max_transparent)
        on_device = type(origins).__module__.split(".")[0] == "torch" and getattr(origins, "is_cuda", False)
        if on_device:
            import torch
            dev = origins.device
            count = int(origins.shape[0])

            def vec(a, dt, shape):
                if a is None:
                    return None
                if a.device != dev or a.dtype != dt or not a.is_contiguous() or tuple(a.shape) != shape:
                    raise ValueError("device arrays of a ray query must be contiguous %s tensors of shape %r on %s" % (dt, shape, dev))
                return a

            def new(shape, dt):                # (zeroed on the stream: the rows a query leaves alone read as zeros)
                return torch.zeros(shape, dtype=dt, device=dev)
            ptr = lambda a: None if a is None else a.data_ptr()
            f4, i4 = torch.float32, torch.int32
        else:
            origins = np.ascontiguousarray(origins, f32)
            count = int(origins.shape[0]) if origins.ndim == 2 else -1

            def vec(a, dt, shape):
                if a is None:
                    return None
                a = np.ascontiguousarray(a, dt)
                if a.shape != shape:
                    raise ValueError("expected an array of shape %r, got %r" % (shape, a.shape))
                return a

            def new(shape, dt):
                return np.zeros(shape, dt)
            ptr = lambda a: None if a is None else a.ctypes.data
            f4, i4 = f32, np.int32
        if count < 0 or tuple(origins.shape) != (count, n):
            raise ValueError("origins must have shape (count, %d)" % n)
        rays = _lib.NtRayBatch()
        keep = [vec(origins, f4, (count, n)), vec(directions, f4, (count, n)), vec(t_near, f4, (count,)), vec(t_far, f4, (count,)),
                vec(distance, f4, (count,)), vec(skip_item, i4, (count,)), vec(skip_lane, i4, (count,))]
        if keep[1] is None:
            raise ValueError("directions are required")
        rays.count = count
        (rays.origins, rays.directions, rays.t_near, rays.t_far, rays.distance, rays.skip_item, rays.skip_lane) = [ptr(a) for a in keep]
        res = _lib.NtRayResults()
        hits = new((count, 4), i4)
        no = new((count, n), f4) if normals and not occlusion else None
        nd = new((count, n), f4) if normals and not occlusion else None
        tl = new((count, max_transparent, 4), i4) if max_transparent > 0 else None
        res.hits, res.normal_origin, res.normal_dir, res.transparent = ptr(hits), ptr(no), ptr(nd), ptr(tl)
        res.max_transparent = max_transparent
        L = _lib.lib()
        if on_device:
            opts = _lib.NtRenderOpts()
            opts.device = dev.index if dev.index is not None else -1
            stream = torch.cuda.current_stream(dev).cuda_stream
            fn = L.nt_occludes_rays_device if occlusion else L.nt_intersect_rays_device
            _lib.check(fn(self._handle, C.byref(rays), C.byref(res), C.byref(opts), stream))
        else:
            fn = L.nt_occludes_rays if occlusion else L.nt_intersect_rays
            _lib.check(fn(self._handle, C.byref(rays), C.byref(res), int(device)))
        dist = hits[:, 0].view(f4)
        out = {"n_transparent": hits[:, 3]}
        if occlusion:
            out["blocked"] = dist != 0
        else:
            item = hits[:, 1]
            miss = (item < 0).to(i4) if on_device else (item < 0).astype(i4)
            out.update(dist=dist, lane=hits[:, 2], kind=(item & 3) - 4 * miss, index=(item >> 2) * (1 - miss) - miss)
            if normals:
                out["normal_origin"], out["normal"] = no, nd
        if tl is not None:
            out["transparent"] = tl
        return out

    def intersect_rays(self, origins, directions, t_near=None, t_far=None, skip_item=None, skip_lane=None, normals=False,
                       max_transparent=0, device=-1):
        """KDNode.intersects on the scene's root for `count` rays at once (nt_intersect_rays).  origins / directions
        [count][n] fp32 (directions as given, not normalised), the optional per-ray arrays [count].  numpy arrays in: a dict
        of numpy arrays out -- dist (FLT_MAX: none), kind (-1: none), index, lane, n_transparent, with `normals` also
        normal_origin / normal (rows of rays without an opaque hit stay zero), with max_transparent > 0 also transparent
        [count][max_transparent][4] int32 records (dist's bits, item, lane, 0).  torch tensors on a HIP device in: the
        same as torch tensors, enqueued on the current stream without a copy or a synchronisation."""
        return self._ray_query(False, origins, directions, t_near, t_far, None, skip_item, skip_lane, normals, max_transparent, device)

    def occludes_rays(self, origins, directions, distance=None, t_near=None, t_far=None, skip_item=None, skip_lane=None,
                      max_transparent=0, device=-1):
        """KDNode.occludes for `count` rays at once (nt_occludes_rays): `blocked`, n_transparent and, with
        max_transparent > 0, the transparent hits met on the way."""
        return self._ray_query(True, origins, directions, t_near, t_far, distance, skip_item, skip_lane, False, max_transparent, device)

    def primary_hits(self, width, height, normals=False, device=-1, out=None, table=None, first=0, count=None, frame_stride=None,
                     strict_reference=None):
        """What is under each pixel of a width x height view (nt_primary_hits): the closest opaque hit of every primary ray,
        found the way a render finds it and before anything is shaded.  Returns a PrimaryHits: dist (FLT_MAX: none), item
        (-1: none), kind, index, lane, n_transparent, each [height][width], and with `normals` normal_origin / normal_dir
        [height][width][n] (rows of pixels without an opaque hit stay as they were: zero in arrays made here).

        `device` an int: numpy arrays through host memory, the scene's current camera.  `device` a torch device (or `out`
        given): torch tensors that stay on the device, enqueued on torch's current stream without a synchronisation.  `out`:
        a dict of the caller's own contiguous torch tensors -- "hits" int32 [frames * frame_stride][4], and with `normals`
        "normal_origin" / "normal_dir" float32 [frames * frame_stride][n].  `table` (a render.CameraTable): frames
        [first, first + count) of it in one launch, every array [count][height][width]..., `frame_stride` >= width * height
        records between the frames (torch only: the table lives on a device)."""
        n = self._n
        width, height = int(width), int(height)
        if width < 1 or height < 1:
            raise ValueError("the view must be at least 1 x 1")
        per_frame = width * height
        torch_device = device if type(device).__module__.split(".")[0] == "torch" or isinstance(device, str) else None
        on_device = torch_device is not None or out is not None or table is not None
        L = _lib.lib()
        res = _lib.NtHitBuffers()
        if not on_device:
            hits = np.zeros((per_frame, 4), np.int32)
            no = np.zeros((per_frame, n), f32) if normals else None
            nd = np.zeros((per_frame, n), f32) if normals else None
            ptr = lambda a: None if a is None else a.ctypes.data
            res.hits, res.normal_origin, res.normal_dir = ptr(hits), ptr(no), ptr(nd)
            _lib.check(L.nt_primary_hits(self._handle, width, height, C.byref(res), int(device)))
            return PrimaryHits(self, width, height, None, per_frame, hits, no, nd)
        import torch
        frames = 1
        if table is not None:
            first = int(first)
            frames = table.frames - first if count is None else int(count)
        stride = per_frame if frame_stride is None else int(frame_stride)
        if stride < per_frame or (table is None and stride != per_frame):
            raise ValueError("frame_stride must be at least width * height (and is only taken with a camera table)")
        if out is not None:
            dev = out["hits"].device
        elif torch_device is not None:
            dev = torch.device(torch_device)
        else:
            dev = torch.device("cuda", torch.cuda.current_device() if int(device) < 0 else int(device))

        def buf(key, shape, dt):
            if out is None:
                return torch.zeros(shape, dtype=dt, device=dev)          # (zeroed on the stream)
            a = out[key]
            if a.device != dev or a.dtype != dt or not a.is_contiguous() or tuple(a.shape) != shape:
                raise ValueError("%r must be a contiguous %s tensor of shape %r on %s" % (key, dt, shape, dev))
            return a
        hits = buf("hits", (frames * stride, 4), torch.int32)
        no = buf("normal_origin", (frames * stride, n), torch.float32) if normals else None
        nd = buf("normal_dir", (frames * stride, n), torch.float32) if normals else None
        ptr = lambda a: None if a is None else a.data_ptr()
        res.hits, res.normal_origin, res.normal_dir = ptr(hits), ptr(no), ptr(nd)
        opts = _lib.NtRenderOpts()
        opts.device = dev.index if dev.index is not None else -1
        if strict_reference is None:
            strict_reference = os.environ.get("NTRACER_STRICT_REFERENCE", "0") not in ("", "0")
        opts.strict_reference = 1 if strict_reference else 0
        stream = torch.cuda.current_stream(dev).cuda_stream
        if table is None:
            _lib.check(L.nt_primary_hits_device(self._handle, width, height, C.byref(res), C.byref(opts), stream))
        else:
            _lib.check(L.nt_primary_hits_table_device(self._handle, width, height, C.byref(res), stride, table._h, first, frames,
                                                      C.byref(opts), stream))
        return PrimaryHits(self, width, height, None if table is None else frames, stride, hits, no, nd)

    # ---- attribute surface of ntracer_body.hpp:833-933 ----
    shadows = property(lambda s: s._p["shadows"])
    camera_light = property(lambda s: s._p["camera_light"])
    max_reflect_depth = property(lambda s: s._p["max_reflect_depth"])
    bg_gradient_axis = property(lambda s: s._p["bg_gradient_axis"])
    ambient_color = property(lambda s: s._p["ambient"])
    bg1 = property(lambda s: s._p["bg1"])
    bg2 = property(lambda s: s._p["bg2"])
    bg3 = property(lambda s: s._p["bg3"])
    point_lights = property(lambda s: tuple(s._point_lights))
    global_lights = property(lambda s: tuple(s._global_lights))

    def _push(self, **changes):
        p = dict(self._p)
        p.update(changes)
        pls = changes.get("_pl", self._point_lights)
        gls = changes.get("_gl", self._global_lights)
        n = self._n
        sp = _lib.NtSceneParams()
        sp.shadows = 1 if p["shadows"] else 0
        sp.camera_light = 1 if p["camera_light"] else 0
        sp.max_reflect_depth = int(p["max_reflect_depth"])
        sp.bg_gradient_axis = int(p["bg_gradient_axis"])
        sp.ambient[:] = tuple(p["ambient"])
        sp.bg1[:] = tuple(p["bg1"])
        sp.bg2[:] = tuple(p["bg2"])
        sp.bg3[:] = tuple(p["bg3"])
        pp = np.asarray([list(l.position) for l in pls], f32).reshape(-1, n)
        pc = np.asarray([list(l.color) for l in pls], f32).reshape(-1, 3)
        gd = np.asarray([list(l.direction) for l in gls], f32).reshape(-1, n)
        gc = np.asarray([list(l.color) for l in gls], f32).reshape(-1, 3)
        sp.n_point_lights = len(pls)
        sp.point_light_pos = pp.ctypes.data_as(_lib.f32p)
        sp.point_light_color = pc.ctypes.data_as(_lib.f32p)
        sp.n_global_lights = len(gls)
        sp.global_light_dir = gd.ctypes.data_as(_lib.f32p)
        sp.global_light_color = gc.ctypes.data_as(_lib.f32p)
        _lib.check(_lib.lib().nt_scene_set_params(self._handle, C.byref(sp)))
        for k, v in changes.items():
            if not k.startswith("_"):
                self._p[k] = v
        self._point_lights = list(pls)
        self._global_lights = list(gls)

    def set_shadows(self, v):
        self._push(shadows=bool(v))

    def set_camera_light(self, v):
        self._push(camera_light=bool(v))

    def set_max_reflect_depth(self, v):
        self._push(max_reflect_depth=int(v))

    def set_ambient_color(self, color):
        self._push(ambient=Color._coerce(color))

    def set_background(self, c1, c2=None, c3=None, axis=1):
        c1 = Color._coerce(c1)
        c2 = c1 if c2 is None else Color._coerce(c2)
        c3 = c1 if c3 is None else Color._coerce(c3)
        axis = int(axis)
        if axis < 0 or axis >= self._n:
            raise ValueError('"axis" must be between 0 and one less than the dimension of the scene')
        self._push(bg1=c1, bg2=c2, bg3=c3, bg_gradient_axis=axis)

    def add_light(self, light):
        if isinstance(light, PointLight):
            if light.dimension != self._n:
                raise TypeError("the light must have the same dimension as the scene")
            self._push(_pl=self._point_lights + [light])
        elif isinstance(light, GlobalLight):
            if light.dimension != self._n:
                raise TypeError("the light must have the same dimension as the scene")
            self._push(_gl=self._global_lights + [light])
        else:
            raise TypeError("object must be an instance of PointLight or GlobalLight")

    def set_params_flat(self, p):
        """Apply a parameter dictionary in the layout of the fixtures (tools/gen_golden.py scene_params)."""
        n = self._n
        pls = [PointLight(Vector(n, pos), tuple(col)) for pos, col in
               zip(np.asarray(p["point_light_pos"], f32).reshape(-1, n), np.asarray(p["point_light_color"], f32).reshape(-1, 3))]
        gls = [GlobalLight(Vector(n, d), tuple(col)) for d, col in
               zip(np.asarray(p["global_light_dir"], f32).reshape(-1, n), np.asarray(p["global_light_color"], f32).reshape(-1, 3))]
        if "fov" in p:
            self.set_fov(float(p["fov"]))
        self._push(shadows=bool(p["shadows"]), camera_light=bool(p["camera_light"]),
                   max_reflect_depth=int(p["max_reflect_depth"]), bg_gradient_axis=int(p["bg_gradient_axis"]),
                   ambient=Color._coerce(tuple(float(v) for v in p["ambient"])),
                   bg1=Color._coerce(tuple(float(v) for v in p["bg1"])), bg2=Color._coerce(tuple(float(v) for v in p["bg2"])),
                   bg3=Color._coerce(tuple(float(v) for v in p["bg3"])), _pl=pls, _gl=gls)


def screen_coord_to_ray(cam, x, y, w, h, fov):
    """tracern.screen_coord_to_ray(cam,x,y,w,h,fov): flat_origin_ray_source (tracer.hpp:60-76), fp32."""
    n = cam.dimension
    half_w = f32(w) / f32(2)
    half_h = f32(h) / f32(2)
    fovI = f32(math.tan(f32(fov) / f32(2))) / half_w
    sx = f32(fovI * f32(f32(x) - half_w))
    sy = f32(fovI * f32(f32(y) - half_h))
    v = (cam._axes[2] + cam._axes[0] * sx) - cam._axes[1] * sy
    return Vector._wrap(v).unit()


def cross(vectors):
    """tracern.cross(vectors) -- generalised cross product (geometry.hpp:884-892)."""
    vs = list(vectors)
    return Vector._wrap(builder.cross([v._v if isinstance(v, Vector) else list(v) for v in vs]).astype(f32))


def _clip_overlaps(n, verts, tight, shared, first_free, lo, hi):
    """nt_polytope_clip_box against the box shrunk by a hair: what merely touches the box is left with nothing."""
    v = np.ascontiguousarray(verts, f32)
    t = np.ascontiguousarray(tight, np.uint64)
    scale = max(1.0, float(np.abs(v).max()), float(np.abs(lo).max()), float(np.abs(hi).max()))
    eps = 1e-6 * scale
    l = np.ascontiguousarray(lo + eps, f32)
    h = np.ascontiguousarray(hi - eps, f32)
    if (l >= h).any():
        return False
    r = _lib.check(_lib.lib().nt_polytope_clip_box(n, len(v), v.ctypes.data_as(_lib.f32p), t.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                   shared, first_free, l.ctypes.data_as(_lib.f32p), h.ctypes.data_as(_lib.f32p), None, None))
    return r > 0


def _simplex_tight(n):
    t = np.zeros((n, 3), np.uint64)
    for i in range(n):
        for j in range(n):
            if j != i:
                t[i, j >> 6] |= np.uint64(1) << np.uint64(j & 63)
    return t


class PrimitivePrototype(object):
    """Base of the objects build_kdtree consumes: a primitive plus its bounding box (tracer.hpp:1363-1373)."""
    boundary = None
    primitive = None

    @property
    def dimension(self):
        return self.boundary.dimension

    @property
    def material(self):
        return self.primitive.material

    def _overlaps(self, lo, hi):
        return bool(((self.boundary.start._v < hi) & (self.boundary.end._v > lo)).all())


class TrianglePointData(object):
    """One vertex of a TrianglePrototype: ``point`` and the edge normal that belongs to it (tracer.hpp:1384-1389)."""
    __slots__ = ("point", "edge_normal")

    def __init__(self, point, edge_normal):
        self.point = point
        self.edge_normal = edge_normal

    def __iter__(self):                    # lets callers that expect plain points unpack the coordinates
        return iter(self.point)


def _point_data(tri, pts):
    # vertex 0 belongs to the edge normal that is minus the sum of the others (the barycentric gradients add up to 0)
    first = Vector._wrap(-np.sum([e._v for e in tri.edge_normals], axis=0))
    return tuple(TrianglePointData(Vector._wrap(pts[k]), first if k == 0 else tri.edge_normals[k - 1]) for k in range(len(pts)))


class TrianglePrototype(PrimitivePrototype):
    """tracern.TrianglePrototype(points[,material]) or TrianglePrototype(triangle) -- tracer.hpp:1391-1405,
    ntracer_body.hpp:2680-2760."""

    def __init__(self, points, material=None):
        if isinstance(points, Triangle):
            if material is not None:
                raise TypeError("material is taken from the triangle")
            self.primitive = points
            a = builder.vertices_of(points.p1._v, points.face_normal._v, [e._v for e in points.edge_normals])
        else:
            pts = [list(p) for p in points]
            if material is None:
                raise TypeError("material is required")
            self.primitive = Triangle.from_points(pts, material)
            a = np.asarray(pts, f32)
        n = a.shape[1]
        self.boundary = AABB(n, a.min(axis=0), a.max(axis=0))
        self.face_normal = self.primitive.face_normal
        self.point_data = _point_data(self.primitive, a)

    def _vertices(self):
        return np.asarray([list(pd.point) for pd in self.point_data], f32)

    def _overlaps(self, lo, hi):
        n = self.dimension
        if not PrimitivePrototype._overlaps(self, lo, hi):
            return False
        return _clip_overlaps(n, self._vertices(), _simplex_tight(n), n - 2, n, lo, hi)


class _LaneView(object):
    """x[i] of a batch prototype's per-lane attribute"""
    __slots__ = ("_items",)

    def __init__(self, items):
        self._items = tuple(items)

    def __getitem__(self, i):
        return self._items[i]

    def __len__(self):
        return len(self._items)


class TriangleBatchPointData(object):
    __slots__ = ("point", "edge_normal")

    def __init__(self, point, edge_normal):
        self.point = point
        self.edge_normal = edge_normal


class TriangleBatchPrototype(PrimitivePrototype):
    """tracern.TriangleBatchPrototype(triangle_prototypes | TriangleBatch) -- tracer.hpp:1406-1437: BATCH_SIZE
    triangle prototypes side by side; ``face_normal[i]``, ``point_data[j].point[i]``, ``point_data[j].edge_normal[i]``
    and ``material[i]`` address lane i."""

    def __init__(self, t_prototypes):
        if isinstance(t_prototypes, TriangleBatch):
            protos = [TrianglePrototype(t) for t in t_prototypes]
            self.primitive = t_prototypes
        else:
            protos = list(t_prototypes)
            if len(protos) != BATCH_SIZE or not all(isinstance(p, TrianglePrototype) for p in protos):
                raise ValueError("exactly %d TrianglePrototype instances are required" % BATCH_SIZE)
            self.primitive = TriangleBatch([p.primitive for p in protos])
        n = protos[0].dimension
        if any(p.dimension != n for p in protos):
            raise TypeError("the prototypes must have the same dimension")
        self._protos = tuple(protos)
        self.boundary = AABB(n, np.min([p.boundary.start._v for p in protos], axis=0), np.max([p.boundary.end._v for p in protos], axis=0))
        self.face_normal = _LaneView(p.face_normal for p in protos)
        self.point_data = tuple(TriangleBatchPointData(_LaneView(p.point_data[j].point for p in protos),
                                                       _LaneView(p.point_data[j].edge_normal for p in protos)) for j in range(n))

    @property
    def material(self):
        return _LaneView(p.material for p in self._protos)

    def _overlaps(self, lo, hi):
        return PrimitivePrototype._overlaps(self, lo, hi) and any(p._overlaps(lo, hi) for p in self._protos)


def triangle_prototypes(simplices, material):
    """Many TrianglePrototypes at once from a (count, n, n) array of vertices (not in the reference: its callers
    loop over TrianglePrototype(points, material); this is that loop with the records computed in bulk)."""
    if not isinstance(material, Material):
        raise TypeError("material must be a Material")
    a = np.ascontiguousarray(simplices, f32)
    p1, fn, edges = builder.from_points_records(a)
    n = a.shape[2]
    out = []
    for k in range(len(a)):
        tp = object.__new__(TrianglePrototype)
        tp.primitive = Triangle(p1[k], fn[k], edges[k], material)
        tp.boundary = AABB(n, a[k].min(axis=0), a[k].max(axis=0))
        tp.face_normal = tp.primitive.face_normal
        tp.point_data = _point_data(tp.primitive, a[k])
        out.append(tp)
    return out


class SolidPrototype(PrimitivePrototype):
    """tracern.SolidPrototype(type,position,orientation,material) -- tracer.hpp:1375-1382."""

    def __init__(self, type, position, orientation, material):
        self.primitive = Solid(type, position, orientation, material)
        lo, hi = builder.solid_bounds(type == CUBE, self.primitive.position._v, orientation._m)
        self.boundary = AABB(orientation.dimension, lo, hi)
        self.type = type
        self.position = self.primitive.position
        self.orientation = orientation
        self.inv_orientation = self.primitive.inv_orientation

    def _overlaps(self, lo, hi):
        n = self.dimension
        if not PrimitivePrototype._overlaps(self, lo, hi):
            return False
        o = self.orientation._m.astype(np.float64)
        pos = self.position._v.astype(np.float64)
        if self.type == CUBE:
            # x = O (u + p), u in [-1,1]^n: a parallelotope; vertex facets: bit 2k (+1 for the upper side of axis k)
            signs = np.array([[1.0 if (m >> k) & 1 else -1.0 for k in range(n)] for m in range(1 << n)])
            verts = (signs + pos) @ o.T
            tight = np.zeros((1 << n, 3), np.uint64)
            for m in range(1 << n):
                for k in range(n):
                    bit = 2 * k + ((m >> k) & 1)
                    tight[m, bit >> 6] |= np.uint64(1) << np.uint64(bit & 63)
            return _clip_overlaps(n, verts, tight, n - 1, 2 * n, lo, hi)
        # sphere: minimise |O^-1 x - p|^2 over the box (convex) by projected gradient from the clamped centre
        inv = self.inv_orientation._m.astype(np.float64)
        x = np.clip(o @ pos, lo, hi)
        step = 1.0 / max(1e-12, 2.0 * np.linalg.norm(inv, 2) ** 2)
        for _ in range(200):
            g = 2.0 * inv.T @ (inv @ x - pos)
            x = np.clip(x - step * g, lo, hi)
        return bool(np.linalg.norm(inv @ x - pos) < 1.0 - 1e-9)


def build_kdtree(primitives, extra_threads=-1, **kwds):
    """tracern.build_kdtree(primitives[,extra_threads=-1,*,update_primitives=False]) -> (AABB, KDNode)
    (ntracer_body.hpp:3250-3325, tracer.hpp:2431-2455).  ``extra_threads`` is accepted for compatibility."""
    max_depth = int(kwds.pop("max_depth", builder.KD_DEFAULT_MAX_DEPTH))
    split_threshold = int(kwds.pop("split_threshold", builder.KD_DEFAULT_SPLIT_THRESHOLD))
    kwds.pop("update_primitives", None)
    kwds_flat = bool(kwds.pop("_flat", False))
    traversal_cost = float(kwds.pop("traversal_cost", 0.0) or 0.0)
    intersection_cost = float(kwds.pop("intersection_cost", 0.0) or 0.0)
    if kwds:
        raise TypeError("unexpected keyword argument %r" % next(iter(kwds)))
    protos = list(primitives)
    if not protos:
        raise ValueError("cannot build tree from empty sequence")
    for p in protos:
        if not isinstance(p, PrimitivePrototype):
            raise TypeError("object is not an instance of PrimitivePrototype")
    n = protos[0].dimension
    if any(p.dimension != n for p in protos):
        raise TypeError("the primitive prototypes must all have the same dimension")
    tri = [builder._Item(p.primitive, p.boundary.start._v, p.boundary.end._v, [p._vertices()]) for p in protos
           if isinstance(p, TrianglePrototype)]
    other = [builder._Item(p.primitive, p.boundary.start._v, p.boundary.end._v) for p in protos if not isinstance(p, TrianglePrototype)]
    batches, loose = builder.group_batches(tri, BATCH_SIZE, TriangleBatch)
    items = batches + loose + other
    if kwds_flat:
        return n, items, builder.build_tree_arrays(items, max_depth, split_threshold, traversal_cost, intersection_cost)
    lo, hi, root = builder.build_tree(items, KDLeaf, KDBranch, max_depth, split_threshold, traversal_cost, intersection_cost)
    return AABB(n, lo, hi), root


def build_composite_scene(primitives, extra_threads=-1, **kwds):
    """tracern.build_composite_scene(primitives[,extra_threads=-1,*,update_primitives=False]) -> CompositeScene
    (ntracer_body.hpp:3335-3357).  The tree goes from the native builder's arrays straight into the scene
    description; KDBranch / KDLeaf objects are not made on the way."""
    n, items, (lo, hi, axis, split, left, right, leaf_items, root) = build_kdtree(primitives, extra_threads, _flat=True, **kwds)
    # primitive tables in item order, materials interned by value
    mats, mat_ids = [], {}

    def mat(m):
        k = m._key()
        if k not in mat_ids:
            mat_ids[k] = len(mats)
            mats.append(list(m.color) + list(m.specular) + [m.opacity, m.reflectivity, m.specular_intensity, m.specular_exp])
        return mat_ids[k]

    rl = n * n + n + 1
    codes = np.zeros(len(items), np.int32)
    batch_recs, batch_mats, tri_recs, tri_mats, solid_recs, solid_types, solid_mats = [], [], [], [], [], [], []
    for k, it in enumerate(items):
        p = it.prim
        if isinstance(p, TriangleBatch):
            codes[k] = (len(batch_recs) << 2) | _lib.KIND_BATCH
            batch_recs.append([t._record() for t in p._tris])
            batch_mats.append([mat(t.material) for t in p._tris])
        elif isinstance(p, Triangle):
            codes[k] = (len(tri_recs) << 2) | _lib.KIND_TRIANGLE
            tri_recs.append(p._record())
            tri_mats.append(mat(p.material))
        else:
            codes[k] = (len(solid_recs) << 2) | _lib.KIND_SOLID
            solid_recs.append(np.concatenate([p.orientation._m.ravel(), p.inv_orientation._m.ravel(), p.position._v]))
            solid_types.append(p.type)
            solid_mats.append(mat(p.material))
    d = dict(dimension=n, root=int(root), node_axis=np.asarray(axis, np.int32), node_split=np.asarray(split, f32),
             node_left=np.asarray(left, np.int32), node_right=np.asarray(right, np.int32),
             items=codes[np.asarray(leaf_items, np.int64)] if len(leaf_items) else np.zeros(0, np.int32),
             batch_recs=np.asarray(batch_recs, f32).reshape(-1, BATCH_SIZE, rl), batch_mats=np.asarray(batch_mats, np.int32).reshape(-1, BATCH_SIZE),
             tri_recs=np.asarray(tri_recs, f32).reshape(-1, rl), tri_mats=np.asarray(tri_mats, np.int32),
             solid_recs=np.asarray(solid_recs, f32).reshape(-1, 2 * n * n + n), solid_types=np.asarray(solid_types, np.int32),
             solid_mats=np.asarray(solid_mats, np.int32), materials=np.asarray(mats, f32).reshape(-1, 10),
             aabb_start=np.asarray(lo, f32), aabb_end=np.asarray(hi, f32))
    return CompositeScene.from_flat(n, d)
