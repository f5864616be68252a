/* Stand-in for the header of small helpers that the reference codec's sources include but do not carry.
 * Written for this project; defines only the names those sources use on their host path. */
#ifndef REF_STANDIN_COMMON_H
#define REF_STANDIN_COMMON_H

#include <stdbool.h>
#include <stdint.h>
#include <string.h>

#define BITMASK(nbits) ((1u << (nbits)) - 1u)
#define MEGABYTE(count) ((count) * 1024ul * 1024ul)
#define ALIGN(value, width) ((((value) + (width) - 1) / (width)) * (width))
#define MIN(a, b) ((a) < (b) ? (a) : (b))
#define UNUSED(name) ((void)(name))

#endif
