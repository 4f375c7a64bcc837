"""TEST INFRASTRUCTURE ONLY.  Harnesses in oracle/_ref linked by an older recipe of oracle/Makefile name the library
beside them by the absolute path of the tree they were built in (DT_NEEDED "/<tree>/oracle/_ref/libscs_ref_amdlinsys.so"),
so they do not load once the tree has moved -- and where the reference sources are not readable, `make conform` cannot
relink them.  `fix(ref_dir)` points every such DT_NEEDED entry at the file name alone, which is a suffix of the same
string in .dynstr, so no byte but the entry's offset changes; the harness's RUNPATH ($ORIGIN) then finds the library
beside it.  Entries are rewritten only where that library lies in ref_dir and the RUNPATH holds $ORIGIN."""
import os
import struct

DT_NULL, DT_NEEDED, DT_STRTAB, DT_RPATH, DT_RUNPATH = 0, 1, 5, 15, 29
PT_LOAD, PT_DYNAMIC = 1, 2


def _cstr(buf, off):
    return buf[off:buf.index(b"\0", off)].decode()


def fix_file(path):
    """-> the entries rewritten, as (old, new) pairs"""
    with open(path, "rb") as f:
        buf = bytearray(f.read())
    if buf[:4] != b"\x7fELF" or buf[4] != 2 or buf[5] != 1:  # 64-bit little-endian ELF only
        return []
    phoff, = struct.unpack_from("<Q", buf, 0x20)
    phentsize, phnum = struct.unpack_from("<HH", buf, 0x36)
    loads, dyn = [], None
    for i in range(phnum):
        p_type, _, p_offset, p_vaddr, _, p_filesz, _, _ = struct.unpack_from("<IIQQQQQQ", buf, phoff + i * phentsize)
        if p_type == PT_LOAD:
            loads.append((p_vaddr, p_offset, p_filesz))
        elif p_type == PT_DYNAMIC:
            dyn = (p_offset, p_filesz)
    if dyn is None:
        return []
    entries, strtab_va = [], None
    for off in range(dyn[0], dyn[0] + dyn[1], 16):
        tag, val = struct.unpack_from("<qQ", buf, off)
        if tag == DT_NULL:
            break
        entries.append((off, tag, val))
        if tag == DT_STRTAB:
            strtab_va = val
    strtab = next((o + strtab_va - va for va, o, sz in loads if strtab_va is not None and va <= strtab_va < va + sz), None)
    if strtab is None:
        return []
    paths = [_cstr(buf, strtab + v) for _, t, v in entries if t in (DT_RUNPATH, DT_RPATH)]
    if not any("$ORIGIN" in p.split(":") for p in paths):
        return []
    here = os.path.dirname(os.path.abspath(path))
    done = []
    for off, tag, val in entries:
        if tag != DT_NEEDED:
            continue
        name = _cstr(buf, strtab + val)
        base = os.path.basename(name)
        if "/" in name and os.path.exists(os.path.join(here, base)):
            struct.pack_into("<Q", buf, off + 8, val + len(name) - len(base))
            done.append((name, base))
    if done:
        tmp = path + ".needed_tmp"
        with open(tmp, "wb") as f:
            f.write(buf)
        os.chmod(tmp, os.stat(path).st_mode)
        os.replace(tmp, path)
    return done


def fix(ref_dir):
    """every regular file of ref_dir (not recursive) -> {file name: rewritten entries}"""
    out = {}
    if not os.path.isdir(ref_dir):
        return out
    for fn in sorted(os.listdir(ref_dir)):
        p = os.path.join(ref_dir, fn)
        if os.path.isfile(p) and not os.path.islink(p):
            done = fix_file(p)
            if done:
                out[fn] = done
    return out
