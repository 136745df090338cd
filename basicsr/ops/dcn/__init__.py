from codeformer_amd.dcn import (DeformConv, DeformConvFunction, DeformConvPack, ModulatedDeformConv, ModulatedDeformConvFunction,
                                ModulatedDeformConvPack, deform_conv, modulated_deform_conv)

__all__ = [
    'DeformConv', 'DeformConvPack', 'ModulatedDeformConv', 'ModulatedDeformConvPack', 'deform_conv', 'modulated_deform_conv',
    'DeformConvFunction', 'ModulatedDeformConvFunction'
]
