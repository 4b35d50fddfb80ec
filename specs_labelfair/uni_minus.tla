------------------------------ MODULE uni_minus ------------------------------
(* Written to show: A UNIPROCESS FAIR ALGORITHM WITH A `-` LABEL: Spec gets WF_vars((pc \notin {"b"}) /\ Next), so the behaviour may stutter at `b` for ever.  Termination is VIOLATED; without the `-` it holds. *)
EXTENDS Naturals

(* --fair algorithm uni_minus
variables flag = 0, n = 0;

begin
  a:   n := 1;
  b:-  flag := 1;
end algorithm *)

=============================================================================
