"""qcrypto-ldpc_amd: host-side mirror (Python, ctypes) of the LDPC reconciliation path.

The product is ``libqldpc.so`` (hand-written HIP for gfx950 behind the C ABI of ``include/qldpc.h``).
This package only binds it: names and argument meaning follow the objects the reference harness
builds from AFF3CT (``Decoder_LDPC_BP_flooding(K, N, n_ite, H, info_bits_pos, rule, enable_syndrome,
syndrome_depth, n_frames)``, ``decode_siho``, ``reset``, ``encode`` -- BS/src/main.cpp:172-195,335-393).
PyTorch appears only as the owner of device buffers / streams handed to the C ABI as raw pointers.

There is NO CPU fallback: if the shared library is missing the import fails loudly.

The directory name has a hyphen, so load it with ``_qldpc_loader.load()`` (repo root) which
registers it as module ``qcrypto_ldpc_amd``.
"""
from . import _lib, codes, decoder, qber, hashes, mc, recon, polar, polar_mc, polar_recon

# One module per subsystem, each importing only from _lib and from the modules before it in this list.  The package's names are its
# modules' names, the private ones included: tests and tools reach _L, _chk, the pointer types and a few helpers as attributes of the package.
for _m in (_lib, codes, decoder, qber, hashes, mc, recon, polar, polar_mc, polar_recon):
    globals().update({_k: _v for _k, _v in vars(_m).items() if not _k.startswith("__")})
