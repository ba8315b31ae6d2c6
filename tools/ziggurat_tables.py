#!/usr/bin/env python3
"""Write pyimcom_amd/csrc/ziggurat_tables.h: the three tables of numpy's float64 normal ziggurat (wi_double, ki_double, fi_double, 256
entries each), read as bytes out of the static library that numpy ships in its own wheel, numpy/random/lib/libnpyrandom.a (they are local
symbols of distributions.o).  No numpy source is needed and nothing is computed: the header holds the very bits the installed
``Generator.standard_normal`` uses.  tests/test_noise_host.py checks them against that generator through crafted PCG64 states.

    python tools/ziggurat_tables.py            # rewrites the header
    python tools/ziggurat_tables.py --check    # exit status 1 when the committed header differs
"""

import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "pyimcom_amd", "csrc", "ziggurat_tables.h")
NAMES = ("wi_double", "ki_double", "fi_double")


def archive_members(path):
    """(name, bytes) of every member of a System V ar archive."""
    data = open(path, "rb").read()
    if data[:8] != b"!<arch>\n":
        raise ValueError(f"{path}: not an ar archive")
    pos, longnames = 8, b""
    while pos + 60 <= len(data):
        name = data[pos:pos + 16].decode().rstrip()
        size = int(data[pos + 48:pos + 58])
        body = data[pos + 60:pos + 60 + size]
        if name == "//":
            longnames = body
        elif name not in ("/", "/SYM64/"):
            if name.startswith("/") and name[1:].isdigit():
                start = int(name[1:])
                name = longnames[start:longnames.index(b"\n", start)].decode()
            yield name.rstrip("/"), body
        pos += 60 + size + (size & 1)


def elf_symbols(obj, wanted):
    """{name: bytes} of the defined data symbols `wanted` of a little-endian ELF64 relocatable object."""
    if obj[:6] != b"\x7fELF\x02\x01":
        return {}
    shoff, = struct.unpack_from("<Q", obj, 0x28)
    shentsize, shnum, _ = struct.unpack_from("<HHH", obj, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", obj, shoff + i * shentsize) for i in range(shnum)]
    found = {}
    for sec in secs:
        if sec[1] != 2:  # SHT_SYMTAB
            continue
        stroff = secs[sec[6]][4]
        for i in range(sec[5] // sec[9]):
            st_name, _, _, shndx, value, size = struct.unpack_from("<IBBHQQ", obj, sec[4] + i * sec[9])
            end = obj.index(b"\0", stroff + st_name)
            name = obj[stroff + st_name:end].decode()
            if name in wanted and 0 < shndx < shnum and size:
                start = secs[shndx][4] + value
                found[name] = obj[start:start + size]
    return found


def read_tables():
    lib = os.path.join(os.path.dirname(np.random.__file__), "lib", "libnpyrandom.a")
    for _, body in archive_members(lib):
        syms = elf_symbols(body, NAMES)
        if len(syms) == len(NAMES):
            if any(len(syms[n]) != 2048 for n in NAMES):
                raise ValueError("a ziggurat table of numpy is not 256 x 8 bytes")
            return (np.frombuffer(syms["wi_double"], "<f8"), np.frombuffer(syms["ki_double"], "<u8"), np.frombuffer(syms["fi_double"], "<f8"))
    raise ValueError(f"{lib}: the tables {NAMES} were not found")


NOTICE = """\
// ziggurat_tables.h -- data only: the tables of numpy's float64 normal ziggurat (numpy/random/src/distributions/ziggurat_constants.h:
// wi_double, ki_double, fi_double), written by tools/ziggurat_tables.py from the bytes in numpy %s's libnpyrandom.a.  Do not edit.
// The doubles are hexadecimal floating constants: every bit is numpy's.
//
// The tables are part of NumPy and carry its licence:
//
// Copyright (c) 2005-2024, NumPy Developers.  All rights reserved.
//
// Redistribution and use in source and binary forms, with or without modification, are permitted provided that the following conditions
// are met:
//     * Redistributions of source code must retain the above copyright notice, this list of conditions and the following disclaimer.
//     * Redistributions in binary form must reproduce the above copyright notice, this list of conditions and the following disclaimer
//       in the documentation and/or other materials provided with the distribution.
//     * Neither the name of the NumPy Developers nor the names of any contributors may be used to endorse or promote products derived
//       from this software without specific prior written permission.
//
// THIS SOFTWARE IS PROVIDED BY THE COPYRIGHT HOLDERS AND CONTRIBUTORS "AS IS" AND ANY EXPRESS OR IMPLIED WARRANTIES, INCLUDING, BUT NOT
// LIMITED TO, THE IMPLIED WARRANTIES OF MERCHANTABILITY AND FITNESS FOR A PARTICULAR PURPOSE ARE DISCLAIMED.  IN NO EVENT SHALL THE
// COPYRIGHT OWNER OR CONTRIBUTORS BE LIABLE FOR ANY DIRECT, INDIRECT, INCIDENTAL, SPECIAL, EXEMPLARY, OR CONSEQUENTIAL DAMAGES (INCLUDING,
// BUT NOT LIMITED TO, PROCUREMENT OF SUBSTITUTE GOODS OR SERVICES; LOSS OF USE, DATA, OR PROFITS; OR BUSINESS INTERRUPTION) HOWEVER CAUSED
// AND ON ANY THEORY OF LIABILITY, WHETHER IN CONTRACT, STRICT LIABILITY, OR TORT (INCLUDING NEGLIGENCE OR OTHERWISE) ARISING IN ANY WAY
// OUT OF THE USE OF THIS SOFTWARE, EVEN IF ADVISED OF THE POSSIBILITY OF SUCH DAMAGE.
#pragma once
#ifndef ZIG_TABLE
#define ZIG_TABLE static const  // (ziggurat.hip places the tables in device memory)
#endif
"""


def render():
    wi, ki, fi = read_tables()
    out = [NOTICE % np.__version__]
    for name, typ, vals, fmt in (("ZIG_WI", "double", wi, lambda v: float(v).hex()), ("ZIG_KI", "unsigned long long", ki, lambda v: "0x%016Xull" % int(v)),
                                 ("ZIG_FI", "double", fi, lambda v: float(v).hex())):
        out.append(f"ZIG_TABLE {typ} {name}[256] = {{\n")
        for i in range(0, 256, 4):
            out.append("    " + ", ".join(fmt(v) for v in vals[i:i + 4]) + ",\n")
        out.append("};\n")
    return "".join(out)


if __name__ == "__main__":
    text = render()
    if "--check" in sys.argv[1:]:
        sys.exit(0 if os.path.exists(HEADER) and open(HEADER).read() == text else 1)
    with open(HEADER, "w") as f:
        f.write(text)
    print(HEADER)
