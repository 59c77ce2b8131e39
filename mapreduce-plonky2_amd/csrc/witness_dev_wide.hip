// The device witness executor with the wide block (include/mp2g.h enum mp2g_witness_op_wide): witness_dev.hip compiled a second
// time, into an object of its own (see the head of that file). A program that holds a wide opcode runs witness_exec_kernel_wide
// through witness_exec_launch_wide; every other program runs the kernels of witness_dev.hip.
#define MP2G_WITNESS_WIDE 1
#include "witness_dev.hip"
