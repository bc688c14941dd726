"""The header of a NetCDF-3 file (64-bit offset: version byte 2) in the shape FMS gives its restart files: fixed dimensions and
an unlimited Time with ONE record, axis variables 1 .. n as doubles, and record variables whose data the caller writes itself.

scipy.io.netcdf_file can write such a file, but only from host arrays that it converts itself; pace_amd.util.write_restart has
the variables' data already big-endian and dense in one pinned buffer (pace_restart_pack) and needs to know only where each
variable's bytes go.  The format (NetCDF classic, "File Format Specifications"):

    header   = magic numrecs dim_list gatt_list var_list
    var      = name ndims dimid* vatt_list nc_type vsize begin(8 bytes)
    data     = the fixed variables in the order of their definition, then the records: for each record the record variables in
               the order of their definition, each padded to 4 bytes

`layout()` returns the header's bytes, the bytes of the fixed (axis) variables and, per record variable, its offset in the file.
"""
import struct

import numpy as np

NC_CHAR, NC_FLOAT, NC_DOUBLE = 2, 5, 6
_DIMENSION, _VARIABLE, _ATTRIBUTE = 0x0A, 0x0B, 0x0C
_TYPES = {np.dtype(">f8"): (NC_DOUBLE, 8), np.dtype(">f4"): (NC_FLOAT, 4)}


def _pad(b):
    return b + b"\0" * (-len(b) % 4)


def _name(s):
    b = s.encode("ascii")
    return struct.pack(">i", len(b)) + _pad(b)


def _attributes(attrs):
    """attrs: {name: str}; every attribute of these files is text."""
    if not attrs:
        return struct.pack(">ii", 0, 0)
    out = struct.pack(">ii", _ATTRIBUTE, len(attrs))
    for name, text in attrs.items():
        b = text.encode("ascii")
        out += _name(name) + struct.pack(">ii", NC_CHAR, len(b)) + _pad(b)
    return out


class Variable:
    """name, dims (names; the first of a record variable is the unlimited one), dtype '>f8' or '>f4', attrs {name: text}."""

    def __init__(self, name, dims, dtype, attrs):
        self.name, self.dims, self.dtype, self.attrs = name, tuple(dims), np.dtype(dtype), dict(attrs)


def layout(dimensions, unlimited, global_attrs, variables, axis_values):
    """dimensions: {name: size} in definition order, `unlimited` among them (its size is not used: one record is declared).
    variables: Variables in definition order; axis_values: {name: array} for every variable without the unlimited dimension.
    -> (header bytes, fixed-data bytes that follow the header directly, {record variable: file offset}, file size)."""
    dim_ids = {name: k for k, name in enumerate(dimensions)}
    sizes = []
    for v in variables:
        if v.dtype not in _TYPES:
            raise ValueError(f"{v.name}: a NetCDF-3 restart variable is >f8 or >f4, not {v.dtype}")
        count = 1
        for d in v.dims:
            if d != unlimited:
                count *= int(dimensions[d])
        sizes.append((count * _TYPES[v.dtype][1] + 3) // 4 * 4)

    def header(begins):
        out = b"CDF\x02" + struct.pack(">i", 1)
        out += struct.pack(">ii", _DIMENSION, len(dimensions))
        for name, size in dimensions.items():
            out += _name(name) + struct.pack(">i", 0 if name == unlimited else int(size))
        out += _attributes(global_attrs)
        out += struct.pack(">ii", _VARIABLE, len(variables))
        for v, vsize, begin in zip(variables, sizes, begins):
            out += _name(v.name) + struct.pack(">i", len(v.dims)) + b"".join(struct.pack(">i", dim_ids[d]) for d in v.dims)
            out += _attributes(v.attrs) + struct.pack(">ii", _TYPES[v.dtype][0], vsize) + struct.pack(">q", begin)
        return out

    position = len(header([0] * len(variables)))  # (a begin is 8 bytes whatever its value)
    begins = [0] * len(variables)
    fixed = b""
    for k, v in enumerate(variables):
        if unlimited not in v.dims:
            begins[k] = position
            data = np.ascontiguousarray(axis_values[v.name], dtype=v.dtype).tobytes()
            data = _pad(data)
            assert len(data) == sizes[k]
            fixed += data
            position += sizes[k]
    records = {}
    for k, v in enumerate(variables):
        if unlimited in v.dims:
            begins[k] = records[v.name] = position
            position += sizes[k]
    return header(begins), fixed, records, position
